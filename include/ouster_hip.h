/*
 * ouster_hip.h -- C ABI of the MI355X (gfx950) implementation of the Ouster
 * SDK's per-pixel hot path:
 *     packet-format field decode -> LidarFrame planes, destagger, cartesian.
 *
 * This is the drop-in boundary.  The reference (ouster-sdk 1.0.1) has no C ABI
 * for this path -- its boundary is the C++ API of ouster_core -- so each entry
 * point below names the reference C++ interface it replaces (paths relative to
 * the reference checkout).  The C++ classes in include/ouster/core/ (same names
 * and semantics as the reference: PacketFormat, LidarFrame, FrameBatcher,
 * destagger<T>, XYZLutT<T>, cartesian) are thin host code over these calls; see
 * INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns OUSTER_HIP_OK (0) or a negative error code and
 *     never throws; ouster_hip_last_error() returns a thread-local message.
 *   - all "device" pointers are HIP device pointers on the context's GPU; all
 *     work is ordered on the context's stream (ouster_hip_ctx_stream) and is
 *     asynchronous unless stated otherwise; call ouster_hip_sync() to wait.
 *   - plain pointers and sizes only; no C++/torch types.
 *   - a context is not thread-safe (like the reference's FrameBatcher, one per stream of work,
 *     externally serialised); distinct contexts may be used from distinct threads.  Formats and
 *     LUTs are immutable after creation and may be shared by the calls of their context.
 */
#ifndef OUSTER_HIP_H
#define OUSTER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OUSTER_HIP_OK 0
#define OUSTER_HIP_ERR_INVALID_ARGUMENT (-1) /* maps to std::invalid_argument */
#define OUSTER_HIP_ERR_RUNTIME (-2)          /* HIP runtime failure -> std::runtime_error */
#define OUSTER_HIP_ERR_NO_DEVICE (-3)
#define OUSTER_HIP_ERR_UNSUPPORTED (-4)

#define OUSTER_HIP_MAX_FIELDS 32

/* element type tags == ouster::sdk::core::ChanFieldType
 * (ouster_core/include/ouster/core/chanfield.h:111-128) */
#define OUSTER_HIP_U8 1
#define OUSTER_HIP_U16 2
#define OUSTER_HIP_U32 3
#define OUSTER_HIP_U64 4
#define OUSTER_HIP_I8 5
#define OUSTER_HIP_I16 6
#define OUSTER_HIP_I32 7
#define OUSTER_HIP_I64 8
#define OUSTER_HIP_F32 9
#define OUSTER_HIP_F64 10
#define OUSTER_HIP_F16 12

typedef struct ouster_hip_ctx ouster_hip_ctx;
typedef struct ouster_hip_format ouster_hip_format;
typedef struct ouster_hip_lut ouster_hip_lut;

/* One bit-field: POD mirror of ouster::sdk::core::FieldDecodeInfo
 * (ouster_core/include/ouster/core/field_decode_info.h:24-54):
 *   value = ((*(u64*)(base + offset)) & mask) >> shift   (shift<0: << -shift) */
typedef struct ouster_hip_bits {
    uint64_t mask;
    uint32_t offset;
    int32_t shift;
} ouster_hip_bits;

/* One decoded channel field and the LidarFrame plane it lands in.
 * dst_elem_size = sizeof(plane element) * extra dims (1,2,4,8; 6 for the
 * packed 3 x float16 RGB plane, impl/lidar_frame_impl.h:36-40).  The decoded
 * 64-bit word is truncated little-endian to dst_elem_size bytes exactly as
 * FieldDecodeInfo::get<T> does. */
typedef struct ouster_hip_field_desc {
    ouster_hip_bits bits;    /* offset is relative to the pixel's channel data */
    uint32_t dst_elem_size;
    uint32_t f16_nan_fill;   /* !=0: "zero" for this plane is 0x7e00 per 16-bit lane
                                (ouster_core/src/lidar_frame.cpp:1397-1401) */
} ouster_hip_field_desc;

/* Packet geometry + bit layout: POD mirror of ouster::sdk::core::PacketFormat
 * (ouster_core/include/ouster/core/types.h:137-160, src/parsing.cpp:453-538).
 * Covers the built-in profiles and anything add_custom_profile() registers
 * (ouster_core/include/ouster/core/profile_extension.h:52-55). */
typedef struct ouster_hip_format_desc {
    uint32_t pixels_per_column;   /* H */
    uint32_t columns_per_packet;
    uint32_t columns_per_frame;   /* W */
    uint32_t packet_header_size;
    uint32_t col_header_size;
    uint32_t channel_data_size;
    uint32_t col_footer_size;
    uint32_t packet_footer_size;
    uint32_t col_size;
    uint32_t lidar_packet_size;
    /* column header fields, offsets relative to the column start */
    ouster_hip_bits col_timestamp;
    ouster_hip_bits col_measurement_id;
    ouster_hip_bits col_status;
    /* packet header fields, offsets relative to the packet start */
    ouster_hip_bits frame_id;
    ouster_hip_bits alert_flags;
    ouster_hip_bits thermal_shutdown;
    ouster_hip_bits shot_limiting;
    ouster_hip_bits countdown_thermal_shutdown;
    ouster_hip_bits countdown_shot_limiting;
    uint32_t n_fields;
    uint32_t reserved;
    ouster_hip_field_desc fields[OUSTER_HIP_MAX_FIELDS];
} ouster_hip_format_desc;

/* Sensor calibration for the XYZ lookup table: the arguments of
 * impl::make_xyz_lut (ouster_core/include/ouster/core/xyzlut.h:53-56).
 * Matrices are 4x4 row-major.  n_angles is either H (OS sensors: per-beam
 * angles) or W*H (DF sensors: per-pixel angles, xyzlut.cpp:49-59). */
typedef struct ouster_hip_calib {
    uint32_t w, h;
    double range_unit;
    double beam_to_lidar_transform[16];
    double transform[16];
    const double* azimuth_angles_deg;
    const double* altitude_angles_deg;
    size_t n_angles;
} ouster_hip_calib;

/* frame-level values latched from the first packet of a frame
 * (FrameBatcher::start_frame, ouster_core/src/lidar_frame.cpp:1709-1741) */
typedef struct ouster_hip_frame_meta {
    int64_t frame_id;          /* -1 if the frame has no packets */
    uint64_t frame_status;     /* thermal&0xf | (shot&0xf)<<4, lidar_frame.cpp:1310-1323 */
    uint16_t shutdown_countdown;
    uint16_t shot_limiting_countdown;
    uint32_t n_valid_columns;  /* columns of the frame that received a valid column (not in the reference struct) */
} ouster_hip_frame_meta;

/* Device output pointers of one batched decode.  Every array is dense over
 * the batch: plane i is [n_frames][H][W] elements of fields[i].dst_elem_size
 * bytes, row-major like Field (ouster_core/include/ouster/core/field.h:828-905).
 * Any pointer may be NULL to skip that output. */
typedef struct ouster_hip_frame_out {
    void* planes[OUSTER_HIP_MAX_FIELDS];       /* staggered planes               */
    void* destaggered[OUSTER_HIP_MAX_FIELDS];  /* destagger(plane) fused in       */
    uint64_t* timestamp;        /* [n_frames][W]      LidarFrame::timestamp()      */
    uint16_t* measurement_id;   /* [n_frames][W]      LidarFrame::measurement_id() */
    uint32_t* status;           /* [n_frames][W]      LidarFrame::status()         */
    uint64_t* packet_timestamp; /* [n_frames][W/cpp]  needs host_timestamps        */
    uint8_t* alert_flags;       /* [n_frames][W/cpp]  only touched where a packet exists */
    ouster_hip_frame_meta* frame_meta; /* [n_frames] */
    /* cartesian fused in: xyz[k] = lut(plane of field xyz_field[k]); [n_frames][H*W][3] */
    void* xyz[2];
    int32_t xyz_field[2];       /* index into fields[]; -1 = unused */
    int32_t xyz_dtype;          /* OUSTER_HIP_F32 or OUSTER_HIP_F64 */
    int32_t reserved;
    /* Optional by-product for a range-gated dewarp that follows (ouster_hip_dewarp_frames_counted): how
     * many pixels of every column have gate_min_r <= value <= gate_max_r in the plane of field
     * gate_field (raw range units, like the u32 min_r / max_r of impl/dewarp_impl.h:33-34).  The decode
     * kernel has those values in registers, so the dewarp's counting pass over the RANGE plane
     * disappears.  Layout: u16 [n_frames][OUSTER_HIP_GATE_CHUNKS][W] partial counts (a column's count is
     * the sum over the chunk axis; unused chunks are written as zero).  NULL: not produced. */
    uint16_t* gate_counts;
    uint32_t gate_min_r, gate_max_r;
    int32_t gate_field;         /* index into fields[] of a 32-bit range field */
    int32_t reserved2;
    /* dewarp<T>(points, poses) (ouster_core/include/ouster/core/pose_util.h:38-56) fused behind the
     * cartesian: device array [n_frames][W][16] of row-major 4x4 per-column poses (the frame's
     * body_to_world).  When set, xyz[k] receives R_col * lut(r) + t_col computed in the element type of xyz
     * (the poses are cast to it, as the reference does) while the point is still in registers -- the
     * separate pass over the cloud (read 12 B + write 12 B per point) disappears.  Needs the separable
     * LUT tables (ouster_hip_lut_create).  NULL: xyz stays in the sensor / body frame of the LUT.
     * 16-byte aligned arrays take the wide-tile kernels; an array that is only 8-byte aligned is decoded by the
     * 64-column kernel (same result, slower). */
    const double* xyz_poses;
} ouster_hip_frame_out;
#define OUSTER_HIP_GATE_CHUNKS 8

/* ---- context ------------------------------------------------------------ */
/* stream: an existing hipStream_t to order on (e.g. torch's current stream),
 * OUSTER_HIP_STREAM_NULL to order on the device's null (legacy default) stream,
 * or NULL to let the context create and own a non-blocking stream. */
#define OUSTER_HIP_STREAM_NULL ((void*)(intptr_t)-1)
int ouster_hip_ctx_create(int device, void* stream, ouster_hip_ctx** out);
void ouster_hip_ctx_destroy(ouster_hip_ctx* ctx);
void* ouster_hip_ctx_stream(ouster_hip_ctx* ctx);
int ouster_hip_ctx_device(ouster_hip_ctx* ctx); /* the HIP device ordinal the context was created on */
/* Experiment / test knobs (not part of the behavioural contract; results are identical for every
 * setting).  Their defaults come from OUSTER_HIP_<NAME> environment variables read once in
 * ouster_hip_ctx_create -- the call path itself never touches the environment.
 *   "wide"  -1 auto | 0 k_decode only | 64/128/256/512 force that k_decode_wide tile width
 *   "tile"  force k_decode's tile width (64/32/16)      "wide_kb"  LDS budget of a wide tile
 *   "wide_min_blocks"  smallest launch that may use wide tiles   "tune"  0: no variant timing
 *   "xcd"   0: plain block -> frame mapping   "fast"  0: every frame through the general mapping
 *   "retune" 1: forget the variant tuner's verdicts (a caller that re-allocated its buffers re-learns)
 *   "stream" -1 auto | 0 never | 128/256 force k_decode_stream's tile width   "stream_rows" rows of its tiles
 *   "stream_wait" 0: trust the in-order vmcnt instead of draining it before a prefetched tile is used
 *   "stream_min_tiles" tiles per persistent workgroup below which a launch stays on the one-tile kernels
 *   "pose_direct" 1: k_pose_interp stores every lane's own row instead of staging a workgroup's rows in LDS (A/B)
 *   "tonemap_bands" 1 .. 64: workgroups per tile of k_tm_hist (bands of the tile's rows) | 0 the launch's own choice (A/B) */
int ouster_hip_ctx_set_knob(ouster_hip_ctx* ctx, const char* name, int value);
int ouster_hip_sync(ouster_hip_ctx* ctx);
const char* ouster_hip_last_error(void);
const char* ouster_hip_version(void);

/* ---- packet format -> device descriptor ---------------------------------- */
/* Replaces constructing ouster::sdk::core::PacketFormat for device use
 * (ouster_core/src/parsing.cpp:600-626). */
int ouster_hip_format_create(ouster_hip_ctx* ctx, const ouster_hip_format_desc* desc,
                             ouster_hip_format** out);
void ouster_hip_format_destroy(ouster_hip_format* fmt);

/* ---- XYZ lookup table ---------------------------------------------------- */
/* Replaces impl::make_xyz_lut(w,h,range_unit,b2l,transform,az,alt)
 * (ouster_core/src/xyzlut.cpp:11-89).  Per-beam (n_angles == h) calibrations
 * are kept as separable per-beam x per-column tables (the LUT is never
 * materialised on the device); per-pixel calibrations fall back to a full
 * double LUT.  Returns INVALID_ARGUMENT for the same dimension errors the
 * reference throws for (xyzlut.cpp:14-21). */
int ouster_hip_lut_create(ouster_hip_ctx* ctx, const ouster_hip_calib* calib,
                          ouster_hip_lut** out);
/* Replaces XYZLutT<T>(direction, offset, h, w) (xyzlut.h:134-135): adopt
 * caller-provided host arrays [n][3] of dtype F32 or F64 (copied to the device). */
int ouster_hip_lut_create_from_arrays(ouster_hip_ctx* ctx, const void* direction,
                                      const void* offset, uint32_t h, uint32_t w,
                                      int dtype, ouster_hip_lut** out);
/* Host copy of the full double LUT, [w*h][3] each == XYZLut::direction/offset
 * (xyzlut.h:82-89). */
int ouster_hip_lut_export(const ouster_hip_lut* lut, double* direction, double* offset);
void ouster_hip_lut_destroy(ouster_hip_lut* lut);

/* ---- batched decode (+ fused destagger + fused cartesian) ---------------- */
/* Replaces a sequence of FrameBatcher::batch(packet, frame) calls
 * (ouster_core/src/lidar_frame.cpp:1824-1884; pixel work :1422-1576, which
 * calls PacketFormat::block_field / col_field, src/parsing.cpp:628-675),
 * optionally followed by destagger<T>() (impl/lidar_frame_impl.h:733-760) and
 * XYZLutT::operator() (xyzlut.h:139-150) on the result.
 *
 * packets: device buffer laid out [n_frames][slots_per_frame][packet_stride]
 *   bytes; packet_stride >= lidar_packet_size.  packet_counts (nullable: all
 *   slots filled) gives the number of leading slots filled per frame; it may be a
 *   DEVICE array (used in place, values clamped to slots_per_frame; the form to use
 *   under stream capture), a pinned host array (copied on the stream; must stay
 *   unchanged until the call has executed) or a plain host array (copied through the
 *   context's pinned staging before the call returns).  No form synchronises the stream.
 *   Packets of a frame may be in any order; a frame's result is "all planes and
 *   column headers zero, then every received column with status&1 and
 *   measurement_id < W written at its measurement_id" -- the memset-then-scatter
 *   equivalent of the reference's incremental zero-fill.
 *   When two received columns carry the same measurement_id the one later in
 *   the buffer wins (the reference: the one batched later).
 *   Fast path: when slots_per_frame * columns_per_packet == W and slot p holds the
 *   packet with columns [p*cpp, (p+1)*cpp) (what a sensor sends, in order; missing
 *   packets may be left as holes with status 0), no mapping work is done at all; any
 *   other arrangement is detected on the device and redone by a second pass.
 *   The call keeps no state between invocations and can be captured in a HIP graph
 *   and replayed on changed packet contents (do one eager call first: scratch
 *   allocations cannot happen during capture).
 * host_timestamps: device array [n_frames][slots_per_frame] of
 *   Packet::host_timestamp values, or NULL (packet_timestamp is then not written).
 * pixel_shift_by_row: HOST array [H] (needed iff any destaggered[] is set).
 * luts: HOST array of n_luts LUT handles; frame f uses luts[f % n_luts]
 *   (multi-sensor batches interleave sensors); NULL iff no xyz output. */
int ouster_hip_decode(ouster_hip_ctx* ctx, const ouster_hip_format* fmt,
                      const uint8_t* packets, size_t packet_stride,
                      uint32_t slots_per_frame, const uint32_t* packet_counts,
                      uint32_t n_frames, const uint64_t* host_timestamps,
                      const ouster_hip_frame_out* out,
                      const int32_t* pixel_shift_by_row,
                      const ouster_hip_lut* const* luts, uint32_t n_luts);

/* ---- standalone destagger ------------------------------------------------ */
/* Replaces destagger_into<T>(img, pixel_shift_by_row, inverse, out)
 * (impl/lidar_frame_impl.h:733-760, N-d variant :776-811): n_images images of
 * h x w elements of elem_bytes bytes (element = T times trailing dims).
 * shifts: HOST array; n_shifts != h -> INVALID_ARGUMENT ("image height does
 * not match shifts size"). */
int ouster_hip_destagger(ouster_hip_ctx* ctx, const void* src, void* dst, uint32_t h,
                         uint32_t w, uint32_t elem_bytes, const int32_t* shifts,
                         uint32_t n_shifts, int inverse, uint32_t n_images);

/* ---- standalone cartesian ------------------------------------------------ */
/* Replaces impl::cartesianT<T>(points, range, direction, offset)
 * (impl/cartesian.h:36-66) / XYZLutT<T>::operator()(range) / cartesian():
 * range [n_images][h*w] u32 (staggered) -> xyz [n_images][h*w][3] of
 * xyz_dtype (F32 or F64). */
int ouster_hip_cartesian(ouster_hip_ctx* ctx, const ouster_hip_lut* lut,
                         const uint32_t* range, void* xyz, int xyz_dtype,
                         uint32_t n_images);

/* ---- dense dewarp ---------------------------------------------------------- */
/* Replaces dewarp<T>(dewarped, points, poses) (ouster_core/include/ouster/core/pose_util.h:38-56):
 * points [n_images][h*w][3] (row-major pixel order, i = row*w + col) are moved by the pose of
 * their column: p' = R_col * p + t_col.  poses: device array [n_images][w][16] doubles, each a
 * row-major 4x4 (LidarFrame::body_to_world layout, lidar_frame.cpp:350-358).  dtype F32/F64 is
 * the element type of points/dewarped; the arithmetic is done in that type like the
 * reference.  points and dewarped may alias. */
int ouster_hip_dewarp(ouster_hip_ctx* ctx, const void* points, const double* poses, void* dewarped,
                      int dtype, uint32_t h, uint32_t w, uint32_t n_images);

/* ---- range-gated, compacting frame dewarp ---------------------------------- */
/* Replaces dewarp<T>(const LidarFrame&, const XYZLutT<T>&, min_range, max_range) and its FrameSet
 * form with provenance (ouster_core/include/ouster/core/pose_util.h:456-493,
 * impl/dewarp_impl.h:23-115) for a batch of frames resident in HBM.
 *   range     [n_frames][h][w] u32   staggered RANGE planes (h, w taken from the LUTs)
 *   status    [n_frames][w]    u32   column status; timestamp [n_frames][w] u64 (nullable unless
 *                                    timestamps_ns is requested); poses [n_frames][w][16] f64
 *   luts      host array, frame f uses luts[f % n_luts] (one XYZLut per sensor of a FrameSet)
 * Per frame: columns first_valid..last_valid (status & 1, lidar_frame.cpp:907-925), skipping
 * status == 0; rows top to bottom; a point is kept when ceil(min_range*1e3) <= r <=
 * floor(max_range*1e3); xyz = lut(r) (f64 tables, or r*dir+ofs in a user LUT's precision), then
 * p' = R_col*p + t_col evaluated in `dtype` with the pose cast to it.  Frames are concatenated in
 * index order.
 * Outputs (device): points [capacity][3] of dtype; optional frame_idxs / col_idxs [capacity] u32,
 * timestamps_ns [capacity] u64; frame_offsets [n_frames + 1] u64 = exclusive prefix of the kept
 * points per frame (frame_offsets[n_frames] = total).  Points beyond `capacity` are dropped, the
 * offsets still report the full counts: h*w*n_frames is always enough
 * (impl::max_number_of_valid_points, pose_util.cpp:15-29). */
int ouster_hip_dewarp_frames(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                             const uint32_t* range, const uint32_t* status,
                             const uint64_t* timestamp, const double* poses, uint32_t n_frames,
                             double min_range, double max_range, int dtype, void* points,
                             uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                             uint64_t capacity, uint64_t* frame_offsets);

/* The same with the per-column kept counts already known: `gate_counts` as written by an
 * ouster_hip_decode of the same frames with the same gate (ceil(min_range*1e3) / floor(max_range*1e3) on
 * RANGE); the counting kernel is skipped.  gate_counts == NULL is ouster_hip_dewarp_frames. */
int ouster_hip_dewarp_frames_counted(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                                     const uint32_t* range, const uint32_t* status,
                                     const uint64_t* timestamp, const double* poses, uint32_t n_frames,
                                     double min_range, double max_range, int dtype, void* points,
                                     uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                                     uint64_t capacity, uint64_t* frame_offsets, const uint16_t* gate_counts);
/* The same with the poses given the way dewarp<float> uses them: pose_rows [n_frames][w][12] float = rows 0..2 of every
 * column's body_to_world (row-major 3 x 4), already cast to float -- dewarp<T> casts the pose to T before it multiplies
 * (pose_util.h:38-56), so for float output this table IS what the arithmetic sees, at 48 B per column instead of the 128 B
 * of a double 4 x 4 (67 MB -> 25 MB per 256 frames of 2048 columns; a caller that stages poses on the host converts them
 * there).  float output only; gate_counts as above (may be NULL). */
int ouster_hip_dewarp_frames_rows(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                                  const uint32_t* range, const uint32_t* status, const uint64_t* timestamp,
                                  const float* pose_rows, uint32_t n_frames, double min_range, double max_range,
                                  void* points, uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                                  uint64_t capacity, uint64_t* frame_offsets, const uint16_t* gate_counts);
/* The raw gate ouster_hip_dewarp_frames derives from metres: min_r = ceil(min_range*1e3), max_r =
 * floor(max_range*1e3), clamped to u32; returns 0 and sets *empty when nothing can pass. */
int ouster_hip_range_gate(double min_range, double max_range, uint32_t* min_r, uint32_t* max_r, int* empty);

/* ---- OSF field planes -------------------------------------------------------- */
/* The device half of decode_field (ouster_osf/src/png_tools.cpp:664-745) for a batch of encoded
 * LidarFrame fields whose entropy coding the host has already undone (PNG: zlib inflate + scanline
 * filters; ZPNG: zstd): pixel bytes -> typed plane elements, and for PNG planes -- which the OSF
 * writer stored destaggered (png_lidarframe_encoder.cpp:112-125) -- the stagger() back, so that the
 * planes land in the same [H][W] staggered layout ouster_hip_decode produces and
 * ouster_hip_destagger / ouster_hip_cartesian / ouster_hip_dewarp_frames run on them unchanged.
 *   PNG_*   src = h rows of w pixels, unfiltered, no filter bytes.  Value = little-endian composition
 *           of the pixel's bytes; 16-bit samples are stored byte-swapped (png_set_swap in the writer).
 *   ZPNG    src = the zstd-decompressed residuals (thirdparty/zpng/zpng.cpp:101-352): per row and
 *           byte lane a running sum mod 256 of the left deltas; 3- and 4-byte pixels come as colour
 *           planes with the GB-RG transform.  Undone on the device (row-wise prefix sums).  Never
 *           staggered: ZPNG planes are stored as they are.
 * The decoded value is truncated / zero-extended to dst_elem_size like the reference's
 * static_cast<T>.  pixel_shift_by_row: HOST array [h] (needed iff any job is a PNG plane). */
#define OUSTER_HIP_OSF_PNG_GRAY8 1
#define OUSTER_HIP_OSF_PNG_GRAY16 2
#define OUSTER_HIP_OSF_PNG_RGB8 3    /* 24-bit values */
#define OUSTER_HIP_OSF_PNG_RGBA8 4   /* 32-bit values */
#define OUSTER_HIP_OSF_PNG_RGBA16 5  /* 64-bit values */
#define OUSTER_HIP_OSF_ZPNG 6        /* src_pixel_bytes = channels * bytes per channel (1..8); 3 and 4 are planar (colour planes,
                                      * GB-RG), the other sizes interleaved; all of 1..8 are tested (tests/test_gpu_osf_unpack.py) */
typedef struct ouster_hip_osf_plane {
    const void* src;          /* device */
    void* dst;                /* device, [h][w] elements of dst_elem_size bytes */
    uint32_t encoding;        /* OUSTER_HIP_OSF_* */
    uint32_t src_pixel_bytes; /* bytes of one source pixel */
    uint32_t dst_elem_size;   /* 1, 2, 4 or 8 */
    uint32_t flags;           /* OUSTER_HIP_OSF_FLAG_* (0: src holds the pixel bytes) */
} ouster_hip_osf_plane;
/* PNG encodings only: `src` is the INFLATED IDAT stream as libpng sees it -- h scanlines of 1 filter-type byte followed by
 * w * src_pixel_bytes filtered bytes (PNG specification section 9: None / Sub / Up / Average / Paeth) -- and the library
 * reverses the scanline filters on the device (k_osf_png_unfilter, round 5) before it unpacks the pixels.  The caller checks
 * the h filter-type bytes (<= 4: the reference's libpng refuses anything else); the kernel treats an unknown type as None. */
#define OUSTER_HIP_OSF_FLAG_FILTERED 1u
int ouster_hip_osf_unpack(ouster_hip_ctx* ctx, const ouster_hip_osf_plane* planes, uint32_t n_planes,
                          uint32_t h, uint32_t w, const int32_t* pixel_shift_by_row);

/* ---- host containers: memory the GPU reaches in place, frame-at-a-time calls -------------------- */
/* The reference's callers work one frame at a time on HOST containers: destagger<T>(img, shifts)
 * (ouster_core/include/ouster/core/lidar_frame.h:917-919), XYZLutT<T>::operator()(range)
 * (xyzlut.h:139-150), dewarp<T>(points, poses) (pose_util.h:38-56), FrameBatcher::batch(packet, frame)
 * (lidar_frame.h:1043-1144).  For those the cost is the PCIe crossing, not the kernel, so this
 * group removes everything else from it:
 *   - ouster_hip_host_alloc hands out page-locked host memory from a process-wide pool (freed
 *     blocks are kept and handed out again: no hipHostMalloc in steady state).  The GPU reads
 *     and writes such memory IN PLACE: every "device pointer" of this header may be a pointer into a
 *     pool block, and a kernel launched on it moves its input and its output over the full-duplex
 *     link at the same time, in one launch, with no staging copy on either side.  The C++ mirror's
 *     containers (Field, img_t<T>, PointCloudXYZ<T>) allocate from it.
 *   - the *_host entry points take HOST pointers of any provenance and return when the result is
 *     in place: pool memory is used where it lies; other memory (a caller's own Eigen array, a
 *     numpy buffer) goes through grow-only device scratch of the context with asynchronous copies
 *     and ONE stream synchronisation.  Neither route allocates once the context has seen the size.
 * Without a GPU ouster_hip_host_alloc returns plain calloc'd memory (containers still work; every
 * compute entry point fails with OUSTER_HIP_ERR_NO_DEVICE as before). */
#define OUSTER_HIP_HOST_POOL_MIN 2048 /* smaller requests are plain malloc / calloc memory (free() or host_free) */
void* ouster_hip_host_alloc(size_t bytes, int zero);
void ouster_hip_host_free(void* p);
/* 1 when [p, p + bytes) lies inside one live block of the pool (device-accessible), else 0 */
int ouster_hip_host_is_pinned(const void* p, size_t bytes);
/* give cached (free) pool blocks back to the system until at most keep_bytes stay cached */
void ouster_hip_host_pool_trim(size_t keep_bytes);

/* Process-wide allocation counters of this library (device memory: every hipMalloc / hipFree it makes,
 * ouster_hip_device_alloc included; pinned: the pool's hipHostMalloc / hipHostFree calls).  The
 * steady-state contract of the frame-at-a-time calls -- no allocation once the shapes have been
 * seen -- is checked by reading these before and after (tests/cpp/test_core_api.cpp, test_dropin_host_containers). */
typedef struct ouster_hip_alloc_stats {
    uint64_t device_allocs, device_frees;
    uint64_t pinned_allocs, pinned_frees;
    uint64_t pool_requests, pool_hits;       /* host_alloc calls at pool sizes / served from cached blocks */
    uint64_t pool_live_bytes, pool_cached_bytes;
} ouster_hip_alloc_stats;
void ouster_hip_alloc_stats_read(ouster_hip_alloc_stats* out);
/* counted hipMalloc / hipFree on the context's device, for bindings that keep their own device buffers */
int ouster_hip_device_alloc(ouster_hip_ctx* ctx, size_t bytes, void** out);
void ouster_hip_device_free(void* p);

/* destagger_into<T> on host images (impl/lidar_frame_impl.h:733-760): src / dst are HOST pointers. */
int ouster_hip_destagger_host(ouster_hip_ctx* ctx, const void* src, void* dst, uint32_t h, uint32_t w,
                              uint32_t elem_bytes, const int32_t* shifts, uint32_t n_shifts, int inverse);
/* XYZLutT<T>::operator()(range) / cartesianT<T> on host arrays (xyzlut.h:139-150, impl/cartesian.h:36-66) */
int ouster_hip_cartesian_host(ouster_hip_ctx* ctx, const ouster_hip_lut* lut, const uint32_t* range,
                              void* xyz, int xyz_dtype);
/* dewarp<T>(dewarped, points, poses) on host arrays (pose_util.h:38-56); poses [w][16] f64 */
int ouster_hip_dewarp_host(ouster_hip_ctx* ctx, const void* points, const double* poses, void* dewarped,
                           int dtype, uint32_t h, uint32_t w);
/* Asynchronous copies between host memory of any provenance and device memory, ordered on the context's
 * stream; complete after ouster_hip_sync.  (Pool memory: one DMA.  Other memory: the runtime's
 * pageable route, which tools/copybench measures at the pinned rate from 2 MB on.) */
int ouster_hip_copy_in(ouster_hip_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int ouster_hip_copy_out(ouster_hip_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
/* Grow-only device scratch owned by the context (slot 0..7; contents undefined; valid until the same slot is
 * asked for more).  What the *_host calls stage through (0..3); bindings that stage themselves use slots 4..7, and so do the
 * C++ mirror's AutoExposure / BeamUniformityCorrector::update_batch (synchronous: nothing is kept there across calls). */
int ouster_hip_ctx_scratch(ouster_hip_ctx* ctx, uint32_t slot, size_t bytes, void** out);

/* ---- display images: BeamUniformityCorrector / AutoExposure -------------------------------------- */
/* The device half of ouster::sdk::core::image::BeamUniformityCorrector and AutoExposure, single-channel overloads
 * (ouster_core/include/ouster/core/image_processing.h:25-165, src/image_processing.cpp:220-296 and :427-498), batched:
 * n_images images of h x w elements, image i at planes + i * image_stride elements (0: dense, h * w).  in_type is U8, U16,
 * U32 (converted to the image type on load, round to nearest even, like astype / static_cast) or equal to out_type;
 * out_type (F32 / F64) is the type T the reference would be called with: every value below is computed in T, bit for bit.
 * The frame-to-frame state (exponential smoothing, counters, the choice of the map) stays with the caller, in double, as
 * in the reference -- include/ouster/core/image_processing.h holds it.  n_images <= 65535, h * w <= 2^31.
 *
 * ouster_hip_image_dark_rows: the order statistics of compute_dark_count (:427-460).  Over the columns that hold at least one
 *   pixel != 0 (n_cols of them), for every row i >= 1 the n_cols / 2-th smallest of image(i, c) - image(i - 1, c):
 *   medians [n_images][h - 1] of T (all 0 when n_cols == 0), n_cols [n_images] (nullable).
 *   LIMIT: w <= 4096 columns (the kernel keeps one row of keys in LDS).  A wider image is refused with OUSTER_HIP_ERR_UNSUPPORTED
 *   before anything is launched or written; the reference has no such limit.  BeamUniformityCorrector::update / update_batch
 *   then throw std::runtime_error, with the image, the dark counts and the call counter as they were (a call that needs no new
 *   dark counts -- the height is known and it is not the 8th update -- does not reach this function and still succeeds).
 *   ouster_hip_image_percentiles and ouster_hip_image_apply, and so AutoExposure, take any width.
 *   A non-empty image with h < 2 has no row pair: INVALID_ARGUMENT (n_images, h or w == 0: OK, nothing is written).
 * ouster_hip_image_percentiles: the order statistics of AutoExposure::apply (:224-252).  The sample is every 4th element of the
 *   flat image, with `dark` (T [n_images][h], nullable) first corrected to max(x - dark[row], 0), kept when > 0:
 *   n [n_images] = its size, lo_hi [n_images][2] of T = its floor(n * lo_percentile)-th and (n - floor(n * hi_percentile) - 1)-th
 *   smallest values (0, 0 when n == 0).  n < 100 is reported like any other n: the caller decides.
 *   Needs lo_percentile + hi_percentile < 1 and no NaN in the image (the reference is undefined outside this).
 * ouster_hip_image_apply: out(i) = map(max(in(i) - dark[row], 0)) per image: `dark` as above (nullable), maps [n_images] DEVICE
 *   array (nullable: no map).  out may be planes itself when in_type == out_type (in place). */
#define OUSTER_HIP_IMAGE_MAP_NONE 0    /* no map, no clamp to [0, 1]: AutoExposure's early return, or a BeamUniformityCorrector alone */
#define OUSTER_HIP_IMAGE_MAP_SCALE 1   /* x * T(mul), clamped to [0, 1] */
#define OUSTER_HIP_IMAGE_MAP_AFFINE 2  /* ((x - T(sub)) * T(mul)) + T(add), each step rounded, clamped to [0, 1] */
typedef struct ouster_hip_image_map {
    int32_t mode;      /* OUSTER_HIP_IMAGE_MAP_* */
    int32_t use_dark;  /* 0: this image skips the dark-count correction */
    double sub, mul, add;
} ouster_hip_image_map;
int ouster_hip_image_dark_rows(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images,
                               uint32_t h, uint32_t w, size_t image_stride, void* medians, uint32_t* n_cols);
int ouster_hip_image_percentiles(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images,
                                 uint32_t h, uint32_t w, size_t image_stride, const void* dark, double lo_percentile,
                                 double hi_percentile, uint32_t* n, void* lo_hi);
int ouster_hip_image_apply(ouster_hip_ctx* ctx, const void* planes, int in_type, void* out, int out_type, uint32_t n_images,
                           uint32_t h, uint32_t w, size_t in_stride, size_t out_stride, const void* dark,
                           const ouster_hip_image_map* maps);
/* The same on ONE host image of type T (`dtype`, F32 / F64), results in HOST memory when the call returns: pool memory
 * (ouster_hip_host_alloc) is worked on in place, other memory goes through the context's scratch.  dark: HOST T [h] (nullable);
 * map: HOST record (nullable).  ouster_hip_image_apply_host works in place. */
int ouster_hip_image_dark_rows_host(ouster_hip_ctx* ctx, const void* image, int dtype, uint32_t h, uint32_t w, void* medians,
                                    uint32_t* n_cols);
int ouster_hip_image_percentiles_host(ouster_hip_ctx* ctx, const void* image, int dtype, uint32_t h, uint32_t w,
                                      const void* dark, double lo_percentile, double hi_percentile, uint32_t* n,
                                      void* lo_hi);
int ouster_hip_image_apply_host(ouster_hip_ctx* ctx, void* image, int dtype, uint32_t h, uint32_t w, const void* dark,
                                const ouster_hip_image_map* map);

/* ---- display images: the RGB overloads of AutoExposure, LocalToneMapper ------------------------------ */
/* The device half of AutoExposure::update on RGB images (src/image_processing.cpp:307-405) and of LocalToneMapper
 * (:532-710), batched: n_images images of h x w pixels of 3 interleaved elements, image i at images + i * image_stride ELEMENTS
 * (0: dense, 3 * h * w).  in_type is F32 or F64 and then equal to out_type, or F16 with out_type F32: FLOAT16 bit patterns,
 * converted by the reference's integer formula (:59-65: 0 and 0x7e00 give 0, everything else uint32(bits + 0x1C000) << 13 read
 * as a float -- not an IEEE conversion; any pattern gives a finite float).  out_type (F32 / F64) is the type T the reference
 * would run in: every value below is computed in T step by step, bit for bit.  The frame-to-frame state stays with the caller,
 * in double (include/ouster/core/image_processing.h).  n_images <= 65535, h * w <= 2^31; float / double elements must be finite.
 *
 * ouster_hip_image_lum_percentiles: the order statistics of :312-348 / :538-568.  The sample is the luminance
 *   (r * T(0.299) + g * T(0.587)) + b * T(0.114) of pixels 0, 4, 8, ... of the flat pixel index, kept when > 0:
 *   n [n_images] = its size, lo_hi [n_images][2] of T = its floor(n * lo_percentile)-th and (n - floor(n * hi_percentile) - 1)-th
 *   smallest values (0, 0 when n == 0).  n < 100 is reported like any other n.  Needs lo_percentile + hi_percentile < 1.
 *   For the RGB AutoExposure the map that follows is ouster_hip_image_apply over the image seen as h x 3w elements; that call
 *   takes in_type F16 with out_type F32 as well (map NONE: the plain converted image).
 * ouster_hip_image_tonemap: everything of LocalToneMapper::apply after its state machine (:586-689), per image from one record
 *   of the DEVICE array params [n_images]: the map WITHOUT a clamp, dynamic-range compression where `compress`, Reinhard, the
 *   8 x 8 tile tables of 1024 bins (clip limit 1, excess and CDF summed in bin order in float), their bilinear blend
 *   (extrapolating in the outer half tiles, as the reference does) and the saturation pass with
 *   color_factor = T(0.75) * T(color_ramp).  map.mode NONE is the reference's early return: the image is left alone, or
 *   converted / copied when out is another buffer.  out may be images itself when in_type == out_type and the strides agree.
 *   Refused with INVALID_ARGUMENT: NULL pointers, a type pair other than the three above, a stride smaller than an image, and
 *   h < 8 or w < 8 (the reference has empty tiles there and blends NaN tables into the image: a deliberate deviation).
 *   UNSUPPORTED: a tile of more than 2^24 pixels (the reference's float counts stop counting there).
 *   The histograms and tables (2 x 256 KB per image) live in the context's grow-only workspace. */
typedef struct ouster_hip_tonemap_params {
    ouster_hip_image_map map;  /* mode NONE / SCALE / AFFINE with sub, mul, add; use_dark is ignored */
    int32_t compress;          /* 1: hi_state < compress_dr_max_lum */
    int32_t color_correct;     /* 0: scale by lum_clahe / lum_ae only */
    double color_ramp;         /* max(0, (hi_state - 0.5) / 0.5) while hi_state < 1, else 1; the kernel rounds it to T and
                                  multiplies T(0.75) by it, in T as the reference does */
} ouster_hip_tonemap_params;
int ouster_hip_image_lum_percentiles(ouster_hip_ctx* ctx, const void* images, int in_type, int out_type, uint32_t n_images,
                                     uint32_t h, uint32_t w, size_t image_stride, double lo_percentile, double hi_percentile,
                                     uint32_t* n, void* lo_hi);
int ouster_hip_image_tonemap(ouster_hip_ctx* ctx, const void* images, int in_type, void* out, int out_type, uint32_t n_images,
                             uint32_t h, uint32_t w, size_t in_stride, size_t out_stride,
                             const ouster_hip_tonemap_params* params);
/* The same on ONE host image, results in HOST memory when the call returns: pool memory is worked on in place, other memory goes
 * through the context's scratch.  params / map: HOST records.  out may be image itself when the types match.
 * ouster_hip_image_apply_rgb_host is the RGB AutoExposure's second half: ouster_hip_image_apply on the h x 3w view, with the
 * FLOAT16 conversion on load (a NULL map or mode NONE: the converted image, nothing when out == image). */
int ouster_hip_image_lum_percentiles_host(ouster_hip_ctx* ctx, const void* image, int in_type, int out_type, uint32_t h,
                                          uint32_t w, double lo_percentile, double hi_percentile, uint32_t* n, void* lo_hi);
int ouster_hip_image_tonemap_host(ouster_hip_ctx* ctx, const void* image, int in_type, void* out, int out_type, uint32_t h,
                                  uint32_t w, const ouster_hip_tonemap_params* params);
int ouster_hip_image_apply_rgb_host(ouster_hip_ctx* ctx, const void* image, int in_type, void* out, int out_type, uint32_t h,
                                    uint32_t w, const ouster_hip_image_map* map);

/* ---- frame_ops: clip / filter / mask / beam selection ------------------------------------------------ */
/* The device half of ouster::sdk::core::frame_ops (ouster_core/include/ouster/core/frame_ops.h, src/frame_ops.cpp), batched:
 * n_images images of h x w pixels per plane, and a LIST of planes of mixed element types per call (one launch for up to 32
 * planes).  Element types: U8 / U16 / U32 / U64, I8 / I16 / I32 / I64, F32, F64 -- what impl::visit_field_2d visits.
 * n_images <= 65535, h * w <= 2^31; every plane pointer is aligned to its element size.
 *
 * `invalid` is converted like static_cast<T>(invalid) where that is defined: truncated toward zero for an integer type.  A
 * value that does not fit the plane's type after truncation, NaN for an integer type, or a finite value beyond FLT_MAX for
 * F32 (all undefined in the reference) is INVALID_ARGUMENT, and it is checked for EVERY plane before anything is written. */
/* ouster_hip_frame_ops_invalidate only: the plane is a cloud [n_images][h * w][3] of float / double (image_stride in points).
 * The point of an invalidated pixel becomes (0, 0, 0) -- what projection gives for range 0, so a cloud stays
 * ouster_hip_cartesian of its range plane when that plane is invalidated to 0 in the same call.  `invalid` must be 0, no twin. */
#define OUSTER_HIP_FOPS_XYZ_F32 100
#define OUSTER_HIP_FOPS_XYZ_F64 101
typedef struct ouster_hip_fops_plane {
    void* data;           /* image i at data + i * image_stride elements */
    void* twin;           /* invalidate only, nullable: the destaggered copy of the same images (same type and stride); the
                             pixel invalidated at (r, c) is invalidated there at (r, (c + shift[r]) mod w).  Needs pred->shifts */
    size_t image_stride;  /* elements between images; 0: dense (h * w) */
    int32_t type;         /* OUSTER_HIP_U8 ... OUSTER_HIP_F64, or OUSTER_HIP_FOPS_XYZ_* */
    int32_t reserved;
    double invalid;       /* this plane's replacement value */
} ouster_hip_fops_plane;

/* Which pixels ouster_hip_frame_ops_invalidate invalidates.  Evaluated once per pixel, for all planes. */
#define OUSTER_HIP_FOPS_PRED_KEY 1   /* lower <= double(key(r, c)) <= upper: filter_field (BuildFilterMaskOp); a NaN key is kept */
#define OUSTER_HIP_FOPS_PRED_ROWS 2  /* lo <= r < hi: filter_uv "u" */
#define OUSTER_HIP_FOPS_PRED_COLS 3  /* lo <= (c + shift[r]) mod w < hi: filter_uv "v", evaluated on the staggered image */
#define OUSTER_HIP_FOPS_PRED_MASK 4  /* mask(r, c) == 0: mask (ApplyMaskOp); image i uses masks[i % n_masks] */
#define OUSTER_HIP_FOPS_PRED_XYZ 5   /* lower <= double(xyz(r * w + c)[axis]) <= upper: filter_xyz */
typedef struct ouster_hip_fops_pred {
    int32_t kind;          /* OUSTER_HIP_FOPS_PRED_* */
    int32_t src_type;      /* KEY: element type of the key plane; XYZ: OUSTER_HIP_F32 or OUSTER_HIP_F64 */
    const void* src;       /* KEY: [n_images] key planes (may be one of the targets); MASK: [n_masks] u8 masks;
                              XYZ: [n_images][h * w][3] points */
    size_t src_stride;     /* elements (XYZ: points) between images / masks; 0: dense (h * w) */
    uint32_t n_masks;      /* MASK */
    uint32_t axis;         /* XYZ: 0, 1, 2 */
    double lower, upper;   /* KEY / XYZ: value range, inclusive; +-inf allowed */
    uint32_t lo, hi;       /* ROWS / COLS: index range [lo, hi); lo <= hi <= h (ROWS) or w (COLS) */
    const int32_t* shifts; /* HOST [n_shift_tables][h] pixel_shift_by_row tables (any integers): COLS, and every plane with a twin */
    uint32_t n_shift_tables; /* image i uses table i % n_shift_tables (multi-sensor batches interleave sensors) */
    uint32_t reserved;
} ouster_hip_fops_pred;

/* static_cast<T>(invalid) as the bit pattern the kernels write (low bytes of *bits), with the checks above.  Needs no GPU. */
int ouster_hip_frame_ops_invalid_bits(int type, double invalid, uint64_t* bits);
/* ClipOp (frame_ops.cpp:151-163), in place: a value is kept iff lower <= double(v) <= upper (NaN: replaced; u64 / i64 are
 * converted with round-to-nearest-even like the host), else it becomes the plane's `invalid`. */
int ouster_hip_frame_ops_clip(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes,
                              uint32_t n_images, uint32_t h, uint32_t w, double lower, double upper);
/* BuildFilterMaskOp + ApplyMaskOp (frame_ops.cpp:165-207) without the mask image in between: the planes are written only where
 * the predicate holds and are never read (the key plane may be among them: a pixel's predicate is evaluated before its stores). */
int ouster_hip_frame_ops_invalidate(ouster_hip_ctx* ctx, const ouster_hip_fops_pred* pred,
                                    const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t n_images,
                                    uint32_t h, uint32_t w);
/* copy_selected_rows (frame_ops.cpp:134-149): dst[p] [n_images][n_sel][w] = rows indices[] of src[p] [n_images][h][w], elements
 * of elem_bytes[p] bytes (1, 2, 4, 8).  indices: HOST array, every value < h (else INVALID_ARGUMENT); src and dst must not overlap. */
int ouster_hip_frame_ops_select_rows(ouster_hip_ctx* ctx, const void* const* src, void* const* dst,
                                     const uint32_t* elem_bytes, uint32_t n_planes, uint32_t n_images, uint32_t h,
                                     uint32_t w, const uint32_t* indices, uint32_t n_sel);
/* The same on ONE host frame (n_images = 1, dense): every data / src pointer is a HOST pointer, the result is in place when the
 * call returns.  Pool memory (ouster_hip_host_alloc) is worked on where it lies; other memory goes through the context's
 * grow-only scratch (slot 0: the planes, slot 1: the predicate source / the selected rows).  `twin` must be NULL. */
int ouster_hip_frame_ops_clip_host(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h,
                                   uint32_t w, double lower, double upper);
int ouster_hip_frame_ops_invalidate_host(ouster_hip_ctx* ctx, const ouster_hip_fops_pred* pred,
                                         const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w);
int ouster_hip_frame_ops_select_rows_host(ouster_hip_ctx* ctx, const void* const* src, void* const* dst,
                                          const uint32_t* elem_bytes, uint32_t n_planes, uint32_t h, uint32_t w,
                                          const uint32_t* indices, uint32_t n_sel);

/* ---- instrumentation ------------------------------------------------------ */
/* Average duration in ms of the dominant decode kernel over the launches made
 * since the last reset, measured with HIP events on the context's stream
 * (enabled by ouster_hip_timing_enable; adds two event records per timed launch: on == 1 times every launch,
 * on == N > 1 every N-th -- an event pair costs the stream 2 - 3 us, a caller inside a timed region samples). */
int ouster_hip_timing_enable(ouster_hip_ctx* ctx, int on);
int ouster_hip_timing_read(ouster_hip_ctx* ctx, double* avg_ms, uint32_t* n_launches);
/* Tile (columns x rows) of the decode kernel variant the last ouster_hip_decode launched: 64/32/16
 * columns x all rows (k_decode) or 64..512 columns x a row chunk (k_decode_wide).  The variant is
 * picked per workload by timing each candidate twice on the first six calls (knob "tune" = 0 disables
 * that, knob "wide" forces one). */
int ouster_hip_last_decode_tile(ouster_hip_ctx* ctx, int* tile_cols, int* tile_rows);
/* Name of the optimistic-pass kernel the last ouster_hip_decode launched: "k_decode" (64/32/16-column tiles,
 * also every general-mapping launch), "k_decode_wide", or one of the two persistent kernels (tiles double-buffered
 * through LDS-DMA; knob "stream" = 0 disables them, 128 / 256 force that tile width): "k_decode_stream2" (dedicated
 * loader waves, the default) or "k_decode_stream" (every wave fetches; knob "stream_loader" = 0). */
const char* ouster_hip_last_decode_kernel(ouster_hip_ctx* ctx);

/* Persisted verdicts of the variant tuner.  ouster_hip_decode picks its kernel variant per workload shape by timing up to
 * five candidates four times each on the first calls (above); with a cache file a process that finds its workload -- keyed by
 * device (arch, CU count, name), library version, profile, H, W, channel bytes, batch-size class and output set -- launches the
 * recorded variant from its FIRST call and times nothing, and a process that had to measure appends its verdict (one O_APPEND
 * write per verdict: the ranks of one job may share the file).  path NULL or "": no cache (the default; the environment
 * variable OUSTER_HIP_TUNING_CACHE, read in ouster_hip_ctx_create, sets one for every context of the process).  Results do
 * not depend on the variant, only the speed does.  What is NOT persisted: where output buffers live (the placement search of
 * hip::DeviceFrameBatch) -- that is a property of the physical pages an allocation drew, gone with the process. */
int ouster_hip_ctx_set_tuning_cache(ouster_hip_ctx* ctx, const char* path);
/* How the last ouster_hip_decode chose its variant: "cache" (read from the file), "measured" (timed by this context),
 * "measuring" (still timing: the call ran a candidate) or "none" (forced by a knob / a shape with one variant). */
const char* ouster_hip_last_decode_tuner(ouster_hip_ctx* ctx);

/* ---- interp_pose / transform ------------------------------------------------ */
/* Replaces interp_pose (ouster_core/include/ouster/core/pose_util.h:194-434) and transform (:118-173).  Poses are row-major
 * 4x4 doubles.  The known poses travel as host arrays: what is computed once per pair of them -- log(inv(a) b) / (t1 - t0),
 * src/transform_homogeneous.cpp:31-62 -- is done on the host, the per-x work -- a exp((x - t0) scaled_twist),
 * src/transform_vector.cpp:40-60, 96-104 -- on the GPU, always in double; the result is cast to the output type as the
 * reference casts it.  The segment of an x is min(k - 2, #{j >= 1 : x_known[j] <= x}): the first / last segment extrapolate.
 * Validation fails with OUSTER_HIP_ERR_INVALID_ARGUMENT and the reference's message before anything touches the GPU:
 * k < 2, x_known not strictly increasing (every pair is checked), |t1 - t0| < DBL_EPSILON in the pair forms, and -- where x_interp
 * is host memory -- x_interp[i] < x_interp[i - 1] anywhere (a superset of where the reference throws).  x_interp in device
 * memory is not read by the host: every x is evaluated on its own, in any order. */

/* The per-segment table, [k - 1][24] doubles: t0, a[16], scaled_twist[6] (rotation then translation), one pad.  Pure host
 * function, no GPU needed. */
int ouster_hip_pose_segments(const double* x_known, const double* poses_known, uint32_t k, double* segments);
/* The validation alone, pure host as well: the known poses as above and, when x_interp (HOST, n values) is not NULL, that it
 * never decreases.  What the C++ mirror calls before it asks for a GPU. */
int ouster_hip_pose_validate(const double* x_known, const double* poses_known, uint32_t k, const double* x_interp, uint64_t n);
/* x_interp_dev [n] f64 (device) -> poses_out_dev [n][16] of dtype (OUSTER_HIP_F32 / OUSTER_HIP_F64), 16-byte aligned.
 * Asynchronous on the context's stream; n == 0 is a no-op. */
int ouster_hip_interp_pose(ouster_hip_ctx* ctx, const double* x_interp_dev, uint64_t n, const double* x_known,
                           const double* poses_known, uint32_t k, int dtype, void* poses_out_dev);
/* The same on host arrays (pool memory in place, anything else through the context's grow-only scratch); synchronous. */
int ouster_hip_interp_pose_host(ouster_hip_ctx* ctx, const double* x_interp, uint64_t n, const double* x_known,
                                const double* poses_known, uint32_t k, int dtype, void* poses_out);
/* Two known poses, any sign of t1 - t0 (pose_util.h:316-326): every x on the one segment.  Not expressible through the
 * trajectory forms, whose x_known must increase. */
int ouster_hip_interp_pose_pair_host(ouster_hip_ctx* ctx, const double* x_interp, uint64_t n, double t0, const double* x0,
                                     double t1, const double* x1, int dtype, void* poses_out);
/* Per-column poses of frames resident in HBM: timestamp_dev [n_frames][w] u64 ns, status_dev [n_frames][w] u32.  A column
 * with status & 1 gets its pose at double(timestamp) * 1e-9 s into poses_dev [n_frames][w][16] f64 and, when pose_rows_dev is
 * not NULL, float(pose[0..11]) into pose_rows_dev [n_frames][w][12] (the input of ouster_hip_dewarp_frames_rows); the other
 * columns' 128 B and 48 B are left as they are.  One launch, asynchronous. */
int ouster_hip_interp_pose_columns(ouster_hip_ctx* ctx, const uint64_t* timestamp_dev, const uint32_t* status_dev,
                                   uint32_t n_frames, uint32_t w, const double* x_known, const double* poses_known,
                                   uint32_t k, double* poses_dev, float* pose_rows_dev);
/* The column form on two known poses, any sign of t1 - t0 (what DeviceFrameBatch::interp_poses(t0, x0, t1, x1) queues): every
 * valid column on the one segment, outputs and untouched bytes as above. */
int ouster_hip_interp_pose_pair_columns(ouster_hip_ctx* ctx, const uint64_t* timestamp_dev, const uint32_t* status_dev,
                                        uint32_t n_frames, uint32_t w, double t0, const double* x0, double t1,
                                        const double* x1, double* poses_dev, float* pose_rows_dev);
/* transform<T>(transformed, points, pose) (pose_util.h:118-131): R p + t in the points' type (dtype F32 / F64), the pose
 * (16 host doubles) cast to that type first.  points / out [n][3] in device memory, may alias.  Asynchronous. */
int ouster_hip_transform(ouster_hip_ctx* ctx, const void* points_dev, const double* pose16, void* out_dev, int dtype,
                         uint64_t n);
int ouster_hip_transform_host(ouster_hip_ctx* ctx, const void* points, const double* pose16, void* out, int dtype, uint64_t n);

/* ---- algorithm::normals --------------------------------------------------------- */
/* Replaces ouster::sdk::algorithm::normals (ouster_algorithm/src/normals.cpp): unit surface normals of a range image's cloud,
 * one f64 triple per pixel, zero where the pixel has no range or no usable neighbour.  Two launches with one small synchronous
 * round trip between them: k_normals_subtent finds, per frame, the column the reference's compute_vertical_subtent would stop at
 * and leaves the two beams' dot product (16 bytes per frame and return); the host applies clamp, acos and the division with libm
 * (ouster_hip_normals_constants) and hands the constants to k_normals, which evaluates no transcendental function: its result
 * equals a float64 restatement of the reference that rounds every operation on its own, bit for bit.
 * Validation fails with OUSTER_HIP_ERR_INVALID_ARGUMENT and the reference's message before anything touches the GPU. */
typedef struct ouster_hip_normals_consts {
    double px_res_h;    /* 2 pi / (2 pi / w) */
    double px_res_v;    /* 2 pi / subtent */
    double tan_safe;    /* tan(max(min_angle_of_incidence_rad, 1e-6)) */
    double target_sq;   /* target_distance_m squared */
    double subtent;     /* vertical pixel subtent, rad */
} ouster_hip_normals_consts;
/* The constants of one call.  has_pair != 0: the subtent is acos(clamp(dot, -1, 1)) / rows_apart; 0: the reference's fallback,
 * (pi / 2) / max(1, h - 1).  Pure host function, no GPU needed; refuses non-positive target_distance_m /
 * min_angle_of_incidence_rad with the reference's messages. */
int ouster_hip_normals_constants(uint32_t w, uint32_t h, double min_angle_of_incidence_rad, double target_distance_m, int has_pair,
                                 double dot, uint32_t rows_apart, ouster_hip_normals_consts* out);
typedef struct ouster_hip_normals_desc {
    const void* xyz;               /* first return: [n_frames][h * w][3] of xyz_dtype */
    const uint32_t* range;         /*               [n_frames][h][w], mm */
    const void* xyz2;              /* second return; xyz2 == range2 == NULL selects the single-return form */
    const uint32_t* range2;
    double* normals;               /* [n_frames][h * w][3]; every element is written */
    double* normals2;              /* dual form only */
    const int32_t* pixel_shift_by_row; /* HOST, h entries, any sign and size: the inputs are staggered and destaggered pixel (u, v) lies
                                      at column (v - shift[u]) mod w; NULL: the inputs are destaggered */
    const double* sensor_origins;  /* (w, 3), one per destaggered column, shared by the frames; NULL: zeros, or from poses */
    const double* poses;           /* [n_frames][w][16] row-major 4x4: the origin of column v is the translation of
                                      poses[frame][v] * sensor_to_body; NULL: not used.  Ignored when sensor_origins is given */
    const double* sensor_to_body;  /* HOST, [max(1, n_sensor_to_body)][16] doubles: frame f uses matrix f % n_sensor_to_body (a batch
                                      that interleaves the frames of several sensors).  With poses: as above; NULL: identity.
                                      Without poses: every column's origin is the matrix's translation (a body-frame cloud).
                                      Ignored when sensor_origins is given */
    uint64_t xyz_rows, xyz2_rows;  /* points per frame the clouds hold: h * w, or "normals: xyz dimensions mismatch" */
    uint32_t n_frames, h, w;
    uint32_t range2_h, range2_w;   /* shape of range2 (dual form): h, w, or "normals: range2 dimensions mismatch" */
    uint32_t n_origins;            /* rows of sensor_origins where it is given: w, or "normals: sensor_origins size must match ..." */
    uint32_t pixel_search_range;
    uint32_t n_sensor_to_body;     /* matrices in sensor_to_body; 0 counts as 1 */
    int32_t xyz_dtype;             /* OUSTER_HIP_F32 (widened on load, exact) / OUSTER_HIP_F64 */
    int32_t staggered_output;      /* 1 with pixel_shift_by_row: normal i belongs to point i of the staggered cloud; 0: the
                                      destaggered layout of the reference */
    double min_angle_of_incidence_rad, target_distance_m;
} ouster_hip_normals_desc;
/* Every array but the two marked HOST in device memory.  Synchronous (the subtent round trip).  Work is queued on ctx's stream. */
int ouster_hip_normals(ouster_hip_ctx* ctx, const ouster_hip_normals_desc* desc);
/* The same with every array in host memory (pool memory in place, anything else through the context's grow-only scratch). */
int ouster_hip_normals_host(ouster_hip_ctx* ctx, const ouster_hip_normals_desc* desc);

/* ---- voxel down-sampling ---------------------------------------------------------- */
/* Replaces ouster::sdk::core::voxel_downsample_3d / voxel_downsample_xd (ouster_core/src/voxel_hash_map.cpp:312-393) and
 * ouster::sdk::algorithm::voxel_downsample_with_normals (ouster_algorithm/src/voxel_downsample.cpp).  The voxel of a point is
 * int(floor(p * (1.0 / voxel_size))) per axis, over the first three columns.  The result equals a float64 restatement of the
 * reference (tests/voxel_model.py) bit for bit: sums are left folds over a voxel's points in input order, never atomics.
 * Rows come in first-seen order (voxels by the input index of their first contributing point; a voxel's points, where a strategy
 * keeps several, consecutively in admission order); the reference's order is its hash map's iteration order.
 * On the GPU: k_voxel_keys, k_voxel_insert (open addressing over point indices, the smallest index of a voxel wins its slot), a scan
 * and a stable radix sort by voxel id (rocPRIM), k_voxel_reduce and k_voxel_write (k_voxel.hip).  Every intermediate lives in a
 * grow-only workspace of the context; a call ends with one read-back of the row count and a status word.
 * Refused with OUSTER_HIP_ERR_INVALID_ARGUMENT before anything touches the GPU: "max_points_per_voxel must be greater than 0",
 * then "voxel_size must be greater than 0" (also a non-finite one), cols < 3 ("voxel_downsample_xd: frame must be Nx>=3 (x,y,z +
 * optional attributes)"); with normals: cols != 3 ("voxel_downsample_with_normals expects Nx3 inputs") and
 * "voxel_downsample_with_normals voxel_size must be > 0".  Refused by the kernels (same code, no output row written): a
 * non-finite coordinate among the first three columns, or one whose floor(p / voxel_size) no int32 holds, "voxel_downsample:
 * point outside the int32 voxel grid".  With normals, rows with a non-finite point or normal coordinate or a normal no longer
 * than 1e-12 are skipped, as in the reference, and only the rows that remain are held to the grid.
 * More than 2^30 points: OUSTER_HIP_ERR_UNSUPPORTED. */
#define OUSTER_HIP_VOXEL_FIRST_N_POINT 0   /* the values of core::VoxelDownsampleStrategy */
#define OUSTER_HIP_VOXEL_AVERAGE_POINT 1
#define OUSTER_HIP_VOXEL_RANDOM 2
typedef struct ouster_hip_voxel_desc {
    const void* points;            /* [n][row_stride] of dtype; the first `cols` elements of a row take part */
    const double* normals;         /* [n][3] f64, dense; not NULL selects the with-normals form (cols == 3; strategy,
                                      max_points_per_voxel and min_pts_threshold are not read) */
    double* out;                   /* [out_capacity][cols] f64, dense */
    double* out_normals;           /* [out_capacity][3] f64: the with-normals form's unit normals */
    uint64_t n;                    /* points; 0: *n_out = 0 and nothing else is looked at (without normals) */
    uint64_t out_capacity;         /* rows `out` (and `out_normals`) can hold */
    uint64_t row_stride;           /* elements from one input row to the next; 0: dense (cols) */
    uint64_t max_points_per_voxel; /* FIRST_N_POINT, RANDOM: points a voxel keeps */
    uint64_t min_pts_threshold;    /* AVERAGE_POINT: a voxel with fewer points is not emitted */
    double voxel_size;
    uint32_t cols;                 /* 3 + attribute columns */
    int32_t dtype;                 /* of points: OUSTER_HIP_F32 (widened on load, exact) / OUSTER_HIP_F64 */
    int32_t strategy;              /* OUSTER_HIP_VOXEL_* */
    uint32_t table_log2;           /* 0: the hash table gets the smallest power of two >= 2 n slots; otherwise 2^table_log2 slots,
                                      which must exceed n (and table_log2 <= 31), else INVALID_ARGUMENT.  Changes no result */
} ouster_hip_voxel_desc;
/* Every array in device memory.  Synchronous.  *n_out: rows written.  If the result needs more than out_capacity rows, nothing is
 * written, *n_out is the count needed and the call returns OUSTER_HIP_ERR_INVALID_ARGUMENT.  FIRST_N_POINT and RANDOM with
 * max_points_per_voxel > 1 are sequential by nature: OUSTER_HIP_ERR_UNSUPPORTED here, host code in the _host form. */
int ouster_hip_voxel_downsample(ouster_hip_ctx* ctx, const ouster_hip_voxel_desc* desc, uint64_t* n_out);
/* The same with every array in host memory (pool memory in place, anything else through the context's grow-only scratch).  The two
 * combinations the GPU does not take run ouster_hip_voxel_downsample_ref. */
int ouster_hip_voxel_downsample_host(ouster_hip_ctx* ctx, const ouster_hip_voxel_desc* desc, uint64_t* n_out);
/* The plain C++ restatement on host arrays: every strategy, the same validation, refusals, row order and out_capacity rule, one
 * core, no GPU.  table_log2 is not read. */
int ouster_hip_voxel_downsample_ref(const ouster_hip_voxel_desc* desc, uint64_t* n_out);
/* Times of the phases of a call, for measurement (tools/ab/voxel_bench.py).  on != 0: every later ouster_hip_voxel_downsample
 * (and _host) on this context records an event around each phase; 0: none (the default; events cost the stream a few us each). */
#define OUSTER_HIP_VOXEL_PHASES 7   /* table reset + keys, insert, ids (first + scan + ids), sort, segments, reduce (gather + fold +
                                       scan; empty for the row-copy forms), write */
int ouster_hip_voxel_timing(ouster_hip_ctx* ctx, int on);
/* ms[OUSTER_HIP_VOXEL_PHASES] of the last timed call that reached the GPU; INVALID_ARGUMENT when there was none. */
int ouster_hip_voxel_phase_ms(ouster_hip_ctx* ctx, float* ms);

/* ---- ICP: point_to_point_align / point_to_plane_align ---------------------------------------- */
/* Replaces ouster::sdk::algorithm::point_to_point_align / point_to_plane_align (ouster_algorithm/src/align_clouds.cpp:1590-1874):
 * up to 10 passes of nearest-neighbour correspondences in a hash grid of cell max_corr_dist over the target, a Huber weight from
 * the median residual, and a Kabsch (point) or 6x6 Gauss-Newton (plane) step.  tests/icp_model.py restates it in float64; the
 * correspondences, residuals, count and median of a pass equal that model bit for bit.  The sums of a pass are reduced in a tree
 * of fixed shape (a workgroup per run of ouster_hip_icp_chunk_rows() rows: in the thread, across the wave, across waves, then the
 * partials folded in index order): a function of the inputs alone, not the reference's left fold.  No floating-point atomic.
 * On the GPU (k_icp.hip): the target grid once per call (cell table of k_voxel.hip, scan and stable radix sort of rocPRIM, the
 * participating rows gathered in cell order), then per pass k_icp_correspond, a radix sort of the |r| keys for the median, the sum
 * kernels, one read-back, and the solve on the host (host/icp_util.cpp).  Intermediates live in a grow-only workspace of the context.
 * Refused with OUSTER_HIP_ERR_INVALID_ARGUMENT before anything touches the GPU, in the reference's order: "max_corr_dist must be
 * finite and greater than zero"; with normals "max_normal_angle_deg must be finite and in [0, 180]", "source_points and
 * source_normals must have the same number of rows", "target_points and target_normals must have the same number of rows".
 * Normals on one side only: "normals must be given for both clouds or for neither".  Refused by the kernels (same code, the outputs
 * untouched): a participating target coordinate whose cell no int32 holds, "point_to_point_align: target point outside the int32
 * cell grid" ("point_to_plane_align: ..." with normals).  A query whose cell lies outside that grid has no neighbour.
 * Fewer than 20 rows on either side: pose = initial_guess, solved = 0, nothing is launched.  More than 2^30 rows: UNSUPPORTED. */
#define OUSTER_HIP_ICP_SUMS 27   /* point: sum w, w x[3], w q[3], then the 9 of sum w (x - cx)(q - cq)^T row-major (16 used);
                                    plane: the 21 entries a <= b of sum w j j^T row-major, then the 6 of sum -w j r, j = (x cross n, n) */
typedef struct ouster_hip_icp_desc {
    const void* source_points;     /* [n_source][source_stride] of dtype */
    const void* target_points;     /* [n_target][target_stride] of dtype */
    const void* source_normals;    /* [n_source_normals][source_normal_stride] of dtype, or NULL; both NULL: point to point */
    const void* target_normals;    /* [n_target_normals][target_normal_stride] of dtype, or NULL */
    uint64_t n_source, n_target;
    uint64_t n_source_normals, n_target_normals;   /* rows of the normals: must equal n_source / n_target */
    uint64_t source_stride, target_stride, source_normal_stride, target_normal_stride;   /* elements per row; 0: 3 */
    int32_t dtype;                 /* of all four arrays: OUSTER_HIP_F32 (widened on load, exact) / OUSTER_HIP_F64 */
    int32_t reserved;
    double initial_guess[16];      /* row-major 4x4 */
    double max_corr_dist;
    double max_normal_angle_deg;   /* read with normals only */
    /* results */
    double pose[16];               /* row-major 4x4; initial_guess where solved == 0 */
    uint32_t iterations;           /* passes of the loop that were run, the one that ended it included */
    uint32_t solved;               /* 1: some pass had at least 20 correspondences */
    uint64_t correspondences;      /* of the last pass */
} ouster_hip_icp_desc;
/* One pass from a given pose, with everything the tests compare. */
typedef struct ouster_hip_icp_step_out {
    int32_t* nn;                   /* [n_source] the neighbour's target row, -1 for none or gated out; NULL: not wanted.  Device
                                      memory for ouster_hip_icp_step, host memory for ouster_hip_icp_step_ref */
    double* r;                     /* [n_source] the residual, 0.0 where nn < 0; NULL: not wanted */
    uint64_t count;                /* correspondences */
    double median;                 /* of |r|; 0 below 20 correspondences, like everything that follows */
    double huber_delta;
    double sums[OUSTER_HIP_ICP_SUMS];
    double centroid_x[3], centroid_q[3];   /* point to point: what the second pass subtracted */
    double next_pose[16];          /* the pose after this pass (the given pose where nothing was solved) */
    int32_t stop;                  /* 1: the loop ends after this pass */
    int32_t solved;                /* 1: the pass had at least 20 correspondences */
} ouster_hip_icp_step_out;
/* Every array in device memory.  Synchronous.  Results in desc->pose / iterations / solved / correspondences. */
int ouster_hip_icp_align(ouster_hip_ctx* ctx, ouster_hip_icp_desc* desc);
/* The same with every array in host memory (pool memory in place, anything else through the context's grow-only scratch). */
int ouster_hip_icp_align_host(ouster_hip_ctx* ctx, ouster_hip_icp_desc* desc);
/* The whole algorithm on host arrays on one core, sums as left folds in source order like the reference: no GPU, no context. */
int ouster_hip_icp_align_ref(ouster_hip_icp_desc* desc);
/* One pass from pose16 (row-major) on device clouds; desc's results are not written.  Fewer than 20 rows on either side:
 * INVALID_ARGUMENT. */
int ouster_hip_icp_step(ouster_hip_ctx* ctx, const ouster_hip_icp_desc* desc, const double* pose16, ouster_hip_icp_step_out* out);
/* The same pass on host arrays with left-fold sums. */
int ouster_hip_icp_step_ref(const ouster_hip_icp_desc* desc, const double* pose16, ouster_hip_icp_step_out* out);
/* Rows a workgroup of the sum kernels owns: the partial sums of a pass are those of consecutive runs of this length. */
uint32_t ouster_hip_icp_chunk_rows(void);
/* Times of the phases of a call, for measurement (tools/ab/icp_bench.py), like ouster_hip_voxel_timing. */
#define OUSTER_HIP_ICP_PHASES 4   /* target grid (once); then summed over the passes: correspond, median (count + key sort +
                                     select), sums (both point passes / the plane pass, and their folds) */
int ouster_hip_icp_timing(ouster_hip_ctx* ctx, int on);
/* ms[OUSTER_HIP_ICP_PHASES] of the last timed call that reached the GPU; INVALID_ARGUMENT when there was none. */
int ouster_hip_icp_phase_ms(ouster_hip_ctx* ctx, float* ms);

/* ---- IcpTarget: a resident ICP target and many sources per call ------------------------------- */
/* A project extension: the reference has no such object.  Scan-to-map and frame-to-keyframe align many sources against one target
 * that does not change.  ouster_hip_icp_target_create builds the target's hash grid once (the grid of ouster_hip_icp_align) and
 * keeps what a query reads -- the slots, the gathered rows, their original indices -- in device memory the handle owns;
 * ouster_hip_icp_target_align then aligns K sources against it in lock step: one launch sequence and one read-back per pass for
 * all K, whatever K is.  Every source is cut into the runs of ouster_hip_icp_chunk_rows() rows the single call uses, a workgroup
 * per run, and a source's partial sums are folded in index order: for each source, pose, iterations, solved and correspondences
 * equal bit for bit those of ouster_hip_icp_align called with that source alone, the target's arrays, and the same max_corr_dist,
 * angle and guess; for any K and any order of the sources.  No floating-point atomic.
 * A target's method is fixed by how it was made: with normals it serves point to plane only, without them point to point only
 * (with normals, other target rows take part).  A target of fewer than 20 rows is legal, needs no context and launches nothing:
 * every alignment against it returns each source's guess (solved = 0, iterations = 0).
 * ouster_hip_icp_target_create refuses, before any GPU work and in this order: NULL arguments; "max_corr_dist must be finite and
 * greater than zero"; "target_points and target_normals must have the same number of rows"; "dtype must be F32 or F64"; "flags
 * must be 0"; "a row stride is smaller than 3"; "NULL pointer"; more than 2^30 rows (UNSUPPORTED, "icp: more than 2^30 rows").
 * It synchronises once, so the grid's refusal ("point_to_point_align: target point outside the int32 cell grid", or
 * "point_to_plane_align: ..." with normals) surfaces there, as INVALID_ARGUMENT.  *out is NULL after every failure.
 * ouster_hip_icp_target_align / _step refuse before any launch, with every output of every source untouched: NULL arguments;
 * "icp_target: made by another context"; on a target with normals "max_normal_angle_deg must be finite and in [0, 180]", then
 * per source "source_points and source_normals must have the same number of rows"; "icp_target: source %u has normals and the
 * target has none" / "icp_target: source %u has no normals and the target has them"; "dtype must be F32 or F64"; a stride below
 * 3; NULL points; more than 65 535 sources or more than 2^30 rows in total (UNSUPPORTED).  n_sources == 0 is OK and does nothing.
 * A source of fewer than 20 rows gets its guess back; the others proceed. */
typedef struct ouster_hip_icp_target ouster_hip_icp_target;
typedef struct ouster_hip_icp_target_desc {
    const void* points;            /* [n][stride] of dtype */
    const void* normals;           /* [n_normals][normal_stride] of dtype, or NULL: a point-to-point target */
    uint64_t n, n_normals;         /* n_normals must equal n where normals are given */
    uint64_t stride, normal_stride;   /* elements per row; 0: 3 */
    int32_t dtype;                 /* OUSTER_HIP_F32 / OUSTER_HIP_F64 */
    uint32_t flags;                /* must be 0 */
    double max_corr_dist;
} ouster_hip_icp_target_desc;
typedef struct ouster_hip_icp_target_info {
    uint64_t rows;                 /* rows given */
    uint64_t rows_used;            /* rows that take part (finite; with normals a finite normal longer than 1e-12) */
    uint64_t cells;                /* occupied cells of the grid */
    uint64_t device_bytes;         /* device memory the handle owns */
    int32_t has_normals;
    int32_t reserved;
    double max_corr_dist;
} ouster_hip_icp_target_info;
typedef struct ouster_hip_icp_source {
    const void* points;            /* [n][stride] of the call's dtype */
    const void* normals;           /* [n_normals][normal_stride], or NULL */
    uint64_t n, n_normals;
    uint64_t stride, normal_stride;   /* elements per row; 0: 3 */
    double initial_guess[16];      /* row-major 4x4 */
    /* results (ouster_hip_icp_target_align), as in ouster_hip_icp_desc */
    double pose[16];
    uint32_t iterations;
    uint32_t solved;
    uint64_t correspondences;
} ouster_hip_icp_source;
/* Arrays in device memory.  ctx may be NULL for a target of fewer than 20 rows. */
int ouster_hip_icp_target_create(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* desc, ouster_hip_icp_target** out);
/* The same with the arrays in host memory (staged like every _host call). */
int ouster_hip_icp_target_create_host(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* desc, ouster_hip_icp_target** out);
/* NULL: nothing. */
void ouster_hip_icp_target_destroy(ouster_hip_icp_target* target);
int ouster_hip_icp_target_info_read(const ouster_hip_icp_target* target, ouster_hip_icp_target_info* info);
/* sources[n_sources], every array in device memory, all of `dtype` (which may differ from the target's).  Synchronous. */
int ouster_hip_icp_target_align(ouster_hip_ctx* ctx, const ouster_hip_icp_target* target, ouster_hip_icp_source* sources,
                                uint32_t n_sources, int32_t dtype, double max_normal_angle_deg);
/* The same with every array in host memory. */
int ouster_hip_icp_target_align_host(ouster_hip_ctx* ctx, const ouster_hip_icp_target* target, ouster_hip_icp_source* sources,
                                     uint32_t n_sources, int32_t dtype, double max_normal_angle_deg);
/* One pass for every source, source k from poses[k] (16 doubles each, row-major), into outs[k] like ouster_hip_icp_step (nn and r:
 * device arrays of that source's rows, or NULL).  The sources' results are not written.  A source or a target of fewer than 20
 * rows: INVALID_ARGUMENT "icp_step: fewer than 20 rows". */
int ouster_hip_icp_target_step(ouster_hip_ctx* ctx, const ouster_hip_icp_target* target, const ouster_hip_icp_source* sources,
                               uint32_t n_sources, int32_t dtype, double max_normal_angle_deg, const double* poses,
                               ouster_hip_icp_step_out* outs);
/* The chunk table of the many-source route for sources of rows[k] rows (0: no chunk), as {source, first row within the source,
 * rows} triples in chunks[cap][3]; returns the number of chunks (more than cap: only cap were written).  Plain host code. */
uint64_t ouster_hip_icp_chunk_table(const uint64_t* rows, uint32_t n_sources, uint32_t* chunks, uint64_t cap);

/* ---- VoxelHashMap3d: a resident, updatable voxel map ------------------------------------------ */
/* Replaces ouster::sdk::core::VoxelHashMap3d (ouster_core/include/ouster/core/voxel_hash_map.h:352-516,
 * ouster_core/src/voxel_hash_map.cpp:13-226; Vector3i / Vector3d / DefaultVoxelBucket / first_n_point).  Every result equals
 * tests/voxel_map_model.py bit for bit.  The handle owns dense arrays indexed by voxel id -- the id is the creation order: cell,
 * count, max_points_per_voxel points of 3 doubles -- and an open-addressing table of voxel ids with a power of two of slots, at
 * least twice the voxel capacity (k_voxel_map.hip).  The arrays grow by doubling once a call's new voxels are counted and before
 * anything is published; a removal compacts into a second set of arrays of the same capacity and rebuilds the table.  Per-call
 * intermediates live in the context's voxel workspace.  No floating-point atomic.  Calls on one map are synchronous and not
 * thread-safe.
 * Deviations from the reference: rows of _pointcloud and _extract_far come voxel by voxel in creation order (earlier calls first,
 * first-seen input order within a call), a voxel's points in admission order, survivors of a removal in their old order (the
 * reference: its hash map's iteration order); a squared distance is ((dx dx + dy dy) + dz dz) (Eigen leaves the order open);
 * _update checks its position before it adds; and what is undefined there is refused or defined here, below.
 * ouster_hip_voxel_map_create refuses, before any GPU work and in this order: NULL arguments; "max_points_per_voxel must be greater
 * than 0"; "voxel_size must be greater than 0" (also a non-finite one); "max_distance must be greater than 0" (also a non-finite
 * one); "num_attributes must be 0 for a fixed-size PointType"; "voxel map: max_distance / voxel_size exceeds the int32 voxel grid"
 * (ceil(max_distance / voxel_size) + 1 above 2^31 - 1); unknown flags; a NULL ctx without OUSTER_HIP_VOXEL_MAP_HOST.
 * _add_points / _update refuse before any GPU work: NULL map; "dtype must be F32 or F64"; "row_stride is smaller than 3"; (update)
 * a position outside the grid, "voxel map: point outside the int32 voxel grid"; n == 0 does nothing; a NULL array; more than 2^30
 * rows (UNSUPPORTED).  Refused by the kernels with the map unchanged: a row with a non-finite coordinate or a cell no int32
 * holds, "voxel map: point outside the int32 voxel grid".  _remove_far / _extract_far refuse an origin outside the grid the same
 * way.  An output with too little capacity writes nothing, changes nothing, reports the rows needed in *n_out and returns
 * INVALID_ARGUMENT "voxel map: out_capacity is too small". */
#define OUSTER_HIP_VOXEL_MAP_HOST 1u   /* flags: the map lives in host memory and runs host/voxel_map_util.cpp on one core; needs no
                                          context, and every array of every call is host memory (both forms of a call) */
typedef struct ouster_hip_voxel_map ouster_hip_voxel_map;
typedef struct ouster_hip_voxel_map_desc {
    double voxel_size;
    double max_distance;              /* the reference's default: 100 */
    uint64_t max_points_per_voxel;    /* the reference's default: 20 */
    uint64_t min_pts_threshold;       /* accepted, no effect (as in the reference for this bucket type) */
    uint64_t num_attributes;          /* must be 0 */
    uint32_t flags;                   /* 0 or OUSTER_HIP_VOXEL_MAP_HOST */
    uint32_t reserved;
} ouster_hip_voxel_map_desc;
typedef struct ouster_hip_voxel_map_info {
    uint64_t voxels;                  /* voxels held */
    uint64_t points;                  /* points held */
    uint64_t voxel_capacity;          /* voxels the arrays hold before they grow */
    uint64_t points_per_voxel;        /* max_points_per_voxel */
    uint64_t device_bytes;            /* device memory the handle owns (0 for a host map) */
} ouster_hip_voxel_map_info;
/* ctx may be NULL only with OUSTER_HIP_VOXEL_MAP_HOST.  The context must outlive the map.  *out is NULL after a failure. */
int ouster_hip_voxel_map_create(ouster_hip_ctx* ctx, const ouster_hip_voxel_map_desc* desc, ouster_hip_voxel_map** out);
/* NULL: nothing. */
void ouster_hip_voxel_map_destroy(ouster_hip_voxel_map* map);
/* Forgets every voxel; keeps the capacity. */
int ouster_hip_voxel_map_clear(ouster_hip_voxel_map* map);
/* Room for `voxels` voxels: a later call that stays within it allocates nothing.  Never shrinks. */
int ouster_hip_voxel_map_reserve(ouster_hip_voxel_map* map, uint64_t voxels);
int ouster_hip_voxel_map_info_read(const ouster_hip_voxel_map* map, ouster_hip_voxel_map_info* info);
/* add_points: points[n][row_stride] of dtype in device memory (row_stride 0: 3), taken in input order. */
int ouster_hip_voxel_map_add_points(ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride);
/* The same with the rows in host memory: pool memory in place, anything else through the context's scratch. */
int ouster_hip_voxel_map_add_points_host(ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride);
/* remove_voxels_far_from_location: origin[3] in host memory. */
int ouster_hip_voxel_map_remove_far(ouster_hip_voxel_map* map, const double* origin);
/* extract_voxels_far_from_location: the same, and the erased points to out[out_capacity][3] (device memory); *n_out: their number. */
int ouster_hip_voxel_map_extract_far(ouster_hip_voxel_map* map, const double* origin, double* out, uint64_t out_capacity, uint64_t* n_out);
int ouster_hip_voxel_map_extract_far_host(ouster_hip_voxel_map* map, const double* origin, double* out, uint64_t out_capacity, uint64_t* n_out);
/* update: add_points, then remove_voxels_far_from_location(position). */
int ouster_hip_voxel_map_update(ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride,
                                const double* position);
int ouster_hip_voxel_map_update_host(ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride,
                                     const double* position);
/* pointcloud: every point to out[out_capacity][3]; *n_out: their number. */
int ouster_hip_voxel_map_pointcloud(const ouster_hip_voxel_map* map, double* out, uint64_t out_capacity, uint64_t* n_out);
int ouster_hip_voxel_map_pointcloud_host(const ouster_hip_voxel_map* map, double* out, uint64_t out_capacity, uint64_t* n_out);
/* get_closest_neighbor for queries[q][row_stride] of dtype, one thread each (voxel_hash_map.cpp:158-215 operation for operation: the
 * 27 cells in VOXEL_SHIFTS order, the lower-bound prune, a voxel's points in admission order, replaced on strict <).
 * out_points[q][3], out_dist_sq[q]; no neighbour: (0, 0, 0) and max_distance_sq.  A neighbour cell no int32 holds is skipped; a
 * non-finite query or one outside the grid has no neighbour.  Refused: NULL map; dtype; stride; q > 0 with a NULL array; more than
 * 2^30 queries (UNSUPPORTED). */
int ouster_hip_voxel_map_closest(const ouster_hip_voxel_map* map, const void* queries, int32_t dtype, uint64_t q, uint64_t row_stride,
                                 double max_distance_sq, double* out_points, double* out_dist_sq);
int ouster_hip_voxel_map_closest_host(const ouster_hip_voxel_map* map, const void* queries, int32_t dtype, uint64_t q,
                                      uint64_t row_stride, double max_distance_sq, double* out_points, double* out_dist_sq);

/* ---- ICPRegistration: a cloud aligned to the resident voxel map (mapping::ICPRegistration::align_points_to_map of the reference,
 * ouster_mapping/src/icp_registration.cpp), held to tests/registration_model.py.  A pass is one kernel (k_registration.hip,
 * k_reg_pass): a workgroup of 256 threads owns ouster_hip_icp_chunk_rows() rows; a thread applies the previous pass's estimate to
 * its rows (the moved cloud lives in the context's workspace, 24 bytes a row, and keeps the roundings of every earlier pass), asks
 * the map with the body of ouster_hip_voxel_map_closest, and forms the Geman-McClure weight k^2 / (k + r2)^2 and the 16 terms of the
 * 6 x 6 system; the correspondences never go to memory.  The sums go through the fixed tree of the ICP above (thread, wave
 * butterfly, waves in order, chunks in index order: the bits depend on the inputs only, no floating-point atomic), one header of
 * 16 doubles and the count comes back per pass, and the host solves (one L D L^T without pivoting, a zero pivot gives a zero
 * component), forms the estimate (Sophus's SE3::exp: translational part first, unit quaternion), composes it on the left and stops
 * after the pass whose dx . dx < convergence_criterion^2.
 * Not the reference's: the L D L^T's order (Eigen's pivots); the tree in place of TBB's deterministic reduce; the fixed rounding
 * orders of the model; a non-finite row or one outside the int32 grid has no correspondence and the pass goes on.
 * Refused before anything touches the GPU: NULL map or desc; a dtype other than F32 / F64; a row_stride below 3 (0 means 3); n > 0
 * with NULL rows; more than 2^30 rows (UNSUPPORTED); a non-finite or negative max_distance, kernel_scale or convergence_criterion;
 * unknown flags.  n == 0, an empty map or max_iterations <= 0: the identity, 0 iterations, no launch.
 * On a map made with OUSTER_HIP_VOXEL_MAP_HOST every form runs host/registration_util.cpp on one core with left-fold sums (the
 * _ref form) on rows in host memory and needs no context. */
#define OUSTER_HIP_REG_SUMS 16   /* w, w s[3], j33, w sx sy, j44, w sx sz, w sy sz, j55, w r[3], w (s x r)[3]: SUMS of the model */
typedef struct ouster_hip_registration_desc {
    int32_t max_iterations;        /* in */
    uint32_t flags;                /* in: 0 */
    double convergence_criterion;  /* in */
    double max_distance;           /* in: a correspondence is strictly nearer */
    double kernel_scale;           /* in: k of the weight */
    double pose[16];               /* out: row-major 4 x 4 */
    uint32_t iterations;           /* out: passes run */
    uint32_t converged;            /* out: the last pass met the criterion */
    uint64_t correspondences;      /* out: of the last pass */
} ouster_hip_registration_desc;
/* rows[n][row_stride] in device memory */
int ouster_hip_registration_align(const ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride,
                                  ouster_hip_registration_desc* desc);
/* rows in host memory: pool memory in place, anything else through the context's scratch */
int ouster_hip_registration_align_host(const ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n,
                                       uint64_t row_stride, ouster_hip_registration_desc* desc);
/* One pass with everything a test compares.  A pose here is (qx, qy, qz, qw, tx, ty, tz). */
typedef struct ouster_hip_registration_step_io {
    const void* points;        /* in: [n][row_stride] of dtype */
    uint64_t n, row_stride;
    int32_t dtype;
    int32_t has_estimate;      /* in: apply `estimate` to every row first (what a later pass does); 0: the rows as they are */
    double estimate[7];
    double max_distance, kernel_scale;
    double* moved;             /* out [n][3]: the rows the pass associated */
    uint8_t* flags;            /* out [n]: 1 where the row has a correspondence */
    double* neighbours;        /* out [n][3]: what the map returned ((0, 0, 0): none) */
    double* dist_sq;           /* out [n]: ... and its squared distance (max_distance^2: none) */
    double sums[OUSTER_HIP_REG_SUMS];
    uint64_t count;
    double dx[6];
    double next_estimate[7];   /* exp(dx) */
} ouster_hip_registration_step_io;
/* arrays in device memory; at least one row */
int ouster_hip_registration_step(const ouster_hip_voxel_map* map, ouster_hip_registration_step_io* io);
/* the same pass on a host map with arrays in host memory and left-fold sums */
int ouster_hip_registration_step_ref(const ouster_hip_voxel_map* map, ouster_hip_registration_step_io* io);
/* The reference's public build_linear_system on host arrays sources[n][3], targets[n][3]: left-fold sums; jtj36 row-major with the
 * lower triangle filled and the upper left zero, as the reference leaves it. */
int ouster_hip_build_linear_system_ref(const double* sources, const double* targets, uint64_t n, double kernel_scale, double* jtj36,
                                       double* jtr6);
/* AdaptiveThreshold's arithmetic (adaptive_threshold.cpp): |t| + 2 max_range sin(theta / 2) of a row-major 4 x 4 deviation, theta as
 * Eigen's AngleAxisd(R).angle() gives it. */
double ouster_hip_registration_model_error(const double* deviation16, double max_range);

#ifdef __cplusplus
}
#endif
#endif /* OUSTER_HIP_H */
