// device_batch.h -- device-resident, batched form of the hot path for C++ callers.
//
// The reference API works one host LidarFrame at a time; on a GPU that costs a PCIe round
// trip per frame.  DeviceFrameBatch keeps a batch of frames in HBM end to end:
//     raw packets (device) --decode+destagger+cartesian--> planes / destaggered planes / XYZ (device)
// It is a thin owner of device buffers around ouster_hip_decode (include/ouster_hip.h); results
// can be read back selectively or handed to other device code through the raw pointers.
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ouster/algorithm/align_clouds.h"
#include "ouster/core/image_processing.h"
#include "ouster/core/lidar_frame.h"
#include "ouster/core/voxel_hash_map.h"
#include "ouster/core/xyzlut.h"
#include "ouster/hip/context.h"
#include "ouster/hip/device_buffer.h"
#include "ouster/mapping/icp_registration.h"

struct ouster_hip_format;

namespace ouster {
namespace sdk {
namespace hip {

struct BatchOptions {
    std::vector<std::string> planes;      ///< staggered planes to produce (empty: the profile's defaults)
    std::vector<std::string> destagger;   ///< planes to also produce destaggered
    bool xyz = false;                     ///< project RANGE (and RANGE2 when present)
    bool xyz_f64 = false;                 ///< XYZ element type (default float)
    bool use_extrinsics = true;           ///< fold SensorInfo::sensor_to_body into the LUT
    /// XYZ in the world frame: decode() applies every column's body_to_world pose (upload_poses(); identity
    /// until set) to the point while it is in registers -- dewarp<T>(cartesian(range), poses) of
    /// pose_util.h:38-56 without the separate pass over the cloud.
    bool xyz_world_frame = false;
    /// Treat every packet slot of every frame as filled (missing packets = zeroed slots, whose
    /// columns are invalid by their status word) instead of uploading per-frame packet counts:
    /// keeps decode() free of host synchronisation, for the streaming pipeline (FrameStream).
    bool all_slots = false;
    /// Range gate of the dewarp() that will follow decode(): when set (max >= min), decode() also counts
    /// the gated RANGE pixels per column (they are in registers there) and dewarp(min, max) with the same
    /// gate skips its counting pass over the RANGE planes.
    double gate_min_range = 0.0, gate_max_range = -1.0;
    /// On by default in its FRUGAL form (round 5; round 4 had it opt-in): batches of >= 64 frames settle WHERE their output
    /// buffers live when they are constructed, one DeviceFrameBatch::refine_placement(placement_draws, nullptr,
    /// placement_ballast_bytes) on an all-zero packet buffer (same store pattern).  With the defaults below: two more copies
    /// of the output set back to back, every buffer group kept at the fastest of its three locations -- 0.1 s and a transient
    /// 2 x output set (6.6 GB for 256 dual-return frames); a draw is skipped when it would take more than three quarters of
    /// the free device memory.  What it buys: the decode's store rate differs by 3 - 20 % between allocations of the same
    /// buffers (+8.7 % on the box of profiles/r05).  Set it to false where construction time or the transient
    /// memory matter more; placement_ballast_bytes > 0 / placement_draws = 4 is the thorough (tens of GB) form.
    /// Pointers handed out afterwards stay valid for the life of the batch.
    /// Only a batch that OWNS its context searches (`context` below left empty): the search re-times kernel variants and would
    /// otherwise reset the tuner state of other batches sharing the context.
    bool auto_placement = true;
    int placement_draws = 3;
    size_t placement_ballast_bytes = 0;
    /// Round 6, off by default (2 - 9 s and ~75 GB transient at construction): behind the search above, tune_placement(10, nullptr,
    /// 4 GB) -- ten whole output sets drawn, the memory given back -- and the group-wise search once more.  About one fresh process
    /// in three gets only slow placements for its first allocations (0.645 of the HBM roofline per decode where the same GPU
    /// gives 0.70 - 0.75) and back-to-back draws do not leave them; the group-wise search run again in the memory the whole-set
    /// draws gave back is what finds the fast groups (profiles/r06_latency/placement_notes.txt).  For pipelines
    /// that live long enough to pay for it; needs auto_placement and an owned context like the search above.
    bool placement_thorough = false;
    /// File with the kernel-variant tuner's verdicts of earlier processes (include/ouster_hip.h,
    /// ouster_hip_ctx_set_tuning_cache): a batch that finds its workload there launches the recorded variant from its first
    /// decode() and times nothing; one that has to measure appends its verdict.  Empty: the process-wide
    /// OUSTER_HIP_TUNING_CACHE, if set, else none.
    std::string tuning_cache;
    int device = -1;                      ///< GPU to work on (-1: hip::current_device() of the constructing thread)
    std::shared_ptr<Context> context;     ///< share this context (stream + scratch) instead of owning one
};

/** Display-image state of a batch's sensors (DeviceFrameBatch::render_images): one AutoExposure per sensor and, unless
 *  switched off, one BeamUniformityCorrector in front of it -- what a caller of the reference keeps per sensor next to its
 *  `buc.update(img); ae.update(img)` lines.  The objects are public: construct them differently by assigning. */
struct ImagePipeline {
    explicit ImagePipeline(size_t n_sensors, bool beam_uniformity = true)
        : auto_exposure(n_sensors), beam_uniformity(beam_uniformity ? n_sensors : 0) {}
    std::vector<core::image::AutoExposure> auto_exposure;
    std::vector<core::image::BeamUniformityCorrector> beam_uniformity;   ///< empty: no correction
};

/** Parameters of DeviceFrameBatch::normals: those of algorithm::normals (algorithm/normals.h), with its defaults. */
struct NormalsOptions {
    uint32_t pixel_search_range = 1;
    double min_angle_of_incidence_rad = 1 * 3.14159265358979323846 / 180.0;
    double target_distance_m = 0.025;
    bool dual_return = false;        ///< both returns in one launch, each a source of neighbour candidates for the other
    bool staggered_output = false;   ///< normal i belongs to point i of xyz_device(); false: the reference's destaggered layout
};

/** Parameters of DeviceFrameBatch::align_voxels: those of algorithm::point_to_point_align / point_to_plane_align
 *  (algorithm/align_clouds.h) with the reference's defaults. */
struct AlignOptions {
    double max_corr_dist = 0.25;
    double max_normal_angle_deg = 20.0;   ///< read on the point-to-plane route only
};

/** What DeviceFrameBatch::align_voxels returns. */
struct AlignResult {
    core::mat4d pose = core::mat4d::Identity();   ///< moves the batch's voxel rows onto the target; the guess where !solved
    uint32_t iterations = 0;                      ///< passes that were run
    uint64_t correspondences = 0;                 ///< of the last pass
    bool solved = false;                          ///< some pass had at least 20 correspondences
    bool point_to_plane = false;                  ///< the route taken
};

/** Parameters of DeviceFrameBatch::voxel_downsample: those of core::voxel_downsample_3d (core/voxel_hash_map.h), except that the
 *  default strategy is AVERAGE_POINT. */
struct VoxelOptions {
    core::VoxelDownsampleStrategy strategy = core::VoxelDownsampleStrategy::AVERAGE_POINT;
    size_t max_points_per_voxel = 1;   ///< FIRST_N_POINT / RANDOM; more than 1 is host code and refused on a resident cloud
    size_t min_pts_threshold = 1;      ///< AVERAGE_POINT
};

class DeviceFrameBatch {
   public:
    /** One LUT per sensor; frame f of the batch uses sensor f % sensors.size(). */
    DeviceFrameBatch(const std::vector<core::SensorInfo>& sensors, uint32_t n_frames,
                     const BatchOptions& options);
    DeviceFrameBatch(const core::SensorInfo& sensor, uint32_t n_frames, const BatchOptions& options)
        : DeviceFrameBatch(std::vector<core::SensorInfo>{sensor}, n_frames, options) {}
    ~DeviceFrameBatch();
    DeviceFrameBatch(const DeviceFrameBatch&) = delete;
    DeviceFrameBatch& operator=(const DeviceFrameBatch&) = delete;

    /** The context (GPU, stream) this batch works on: its own unless BatchOptions::context was given. */
    const std::shared_ptr<Context>& context() const { return ctx_; }
    const core::PacketFormat& packet_format() const { return pf_; }
    /** Slot of a frame's packet buffer a lidar packet belongs in: the index of the packet inside its
     *  frame, measurement_id(first column) / columns_per_packet -- its "home" slot, where the decode
     *  kernels find it without any mapping work.  -1: outside the frame (the packet is dropped, as
     *  the reference drops its columns, lidar_frame.cpp:1432-1434). */
    int home_slot(const uint8_t* lidar_packet) const {
        const uint32_t p = pf_.col_measurement_id(pf_.nth_col(0, lidar_packet)) / pf_.columns_per_packet;
        return p < slots_ ? static_cast<int>(p) : -1;
    }
    /** Put a lidar packet into a staging slot (at least lidar_packet_size bytes).  An empty slot takes the packet as it
     *  is.  A slot that already holds a packet -- the same packet sent again -- is merged the way the reference ends up
     *  after batching both (parse_by_col, lidar_frame.cpp:1422-1466): every valid, in-range column of the later packet
     *  replaces the earlier one's, the others stay; the packet-level bytes (header, footer: alert flags, timestamps) are the
     *  later packet's (batch_lidar_packet :1534-1539). */
    void stage_packet(uint8_t* slot, bool occupied, const uint8_t* lidar_packet) const;
    uint32_t n_frames() const { return n_frames_; }
    size_t packet_stride() const { return stride_; }
    uint32_t slots_per_frame() const { return slots_; }

    /** Device buffer for the raw packets, laid out [n_frames][slots_per_frame][packet_stride]. */
    uint8_t* packets_device() { return static_cast<uint8_t*>(d_packets_.data()); }
    /** Copy one frame's packets (host, each lidar_packet_size bytes) into its slots. */
    void upload_frame_packets(uint32_t frame, const std::vector<const uint8_t*>& packets);
    /** The packet buffer was filled on the device (packets in their home slots, missing ones zeroed -- e.g. by a peer
     *  copy, ShardedBatch::scatter): decode() treats every slot of every frame as present. */
    void assume_all_slots_filled() { counts_.assign(n_frames_, slots_); }

    /** Setup-time choice of WHERE the batch's buffers live.  The physical placement of a device allocation
     *  is drawn when it is made and the decode's achieved write rate differs by 10 - 20 % between draws of
     *  the same size (tools/ab/alloc_lottery.py).  A batch allocates once and is reused for
     *  the life of a pipeline, so it can afford to draw: this re-allocates the output buffers `tries` times
     *  (and the packet buffer, contents preserved, up to 6 times), times decode() into each draw and keeps
     *  the fastest.  Output contents are undefined afterwards (decode() again).  Returns the seconds per
     *  decode() of the kept draw; `all_ms` (optional) receives every draw's time in ms, outputs first.
     *  `ballast_bytes_between_draws` of device memory are held between two draws so that the draws scan the
     *  memory instead of its first few GB: which mode a draw gets follows where it lands (tools/ab/ballast.py). */
    double tune_placement(int tries = 16, std::vector<double>* all_ms = nullptr,
                          size_t ballast_bytes_between_draws = size_t{4} << 30);
    /** The cheap form, and what a large batch does by itself when it is constructed (BatchOptions::auto_placement):
     *  the lottery is mostly an interaction between a few heavy output streams (tools/ab/hybrid_sets.py: exchanging
     *  the two XYZ buffers of a slow set for those of a fast one recovers 90 % of the difference, one buffer alone
     *  nothing), and fast / slow regions of the device memory are tens of GB wide: `draws - 1` further copies of the
     *  output set are allocated `ballast_bytes_between_draws` apart, then GROUP BY GROUP -- XYZ clouds, 32-bit planes,
     *  destaggered planes, narrow planes -- decode() is timed with that group's buffers at each location and the fastest
     *  is kept (the buffers the batch has are a candidate too); everything else is freed.  Output contents are undefined
     *  afterwards; device pointers obtained BEFORE the call are invalid.  Returns seconds per decode() of what is kept;
     *  `all_ms`: the first allocation's time, then every candidate's (groups x (draws - 1)). */
    double refine_placement(int draws = 4, std::vector<double>* all_ms = nullptr,
                            size_t ballast_bytes_between_draws = size_t{8} << 30);

    /** Run the fused kernels on everything uploaded so far (asynchronous; sync() to wait). */
    void decode();
    void sync();

    /** Device pointers of the results ([n_frames][H][W] elements; xyz [n_frames][H*W][3]). */
    void* plane_device(const std::string& name);
    void* destaggered_device(const std::string& name);
    void* xyz_device(int return_index);
    uint64_t* timestamp_device() { return static_cast<uint64_t*>(d_ts_.data()); }
    uint16_t* measurement_id_device() { return static_cast<uint16_t*>(d_mid_.data()); }
    uint32_t* status_device() { return static_cast<uint32_t*>(d_status_.data()); }
    size_t plane_bytes_per_frame(const std::string& name) const;
    size_t xyz_bytes_per_frame() const { return static_cast<size_t>(h_) * w_ * 3 * (opt_.xyz_f64 ? 8 : 4); }
    size_t lidar_packet_size() const { return pf_.lidar_packet_size; }
    uint32_t h() const { return h_; }
    uint32_t w() const { return w_; }
    /** Read one frame's result back (synchronous). */
    void download_plane(const std::string& name, uint32_t frame, void* host, bool destaggered = false);
    void download_xyz(int return_index, uint32_t frame, void* host);
    void download_headers(uint32_t frame, uint64_t* timestamp, uint16_t* measurement_id, uint32_t* status);

    /** Display images of the whole decoded batch without leaving HBM: the destaggered plane of `field` (it must be listed in
     *  BatchOptions::destagger -- @throw std::invalid_argument otherwise) of every frame goes through its sensor's
     *  BeamUniformityCorrector (if the pipeline has one) and AutoExposure: frame f belongs to sensor f % sensors, each
     *  sensor's frames are processed in index order with the reference's state machine (core/image_processing.h).  Returns the
     *  device pointer of the result, float [n_frames][h][w], owned by the batch (allocated on the first call for `field`).
     *  Three kernel launches and two small round trips per sensor; synchronous. */
    void* render_images(const std::string& field, ImagePipeline& pipe, bool update_state = true);
    /** One frame's image of the last render_images(field, ...) (h * w floats; synchronous). */
    void download_image(const std::string& field, uint32_t frame, float* host);

    /** frame_ops on the resident batch (core/frame_ops.h; csrc/k_frame_ops.hip): asynchronous on the batch's stream, the whole
     *  batch in one launch (clip and a filter_xyz whose fields follow both clouds: two).  Fields: nullptr (clip / mask: an empty list) = every
     *  staggered plane the batch holds; a listed name the batch does not hold is skipped, as the reference skips a field a
     *  frame lacks (a batch holds pixel planes only).  Every op keeps the batch consistent:
     *   - the destaggered copy (BatchOptions::destagger) of a target gets the same pixels invalidated.  The batch destaggers every
     *     frame with the FIRST sensor's pixel_shift_by_row (as decode() does); filter_uv "v" is defined on that image;
     *   - RANGE / RANGE2 as a target of a batch with XYZ: the invalidated pixels' points become what projection gives for the
     *     new range.  Implemented for invalid == 0 (the point (0, 0, 0): the cloud equals ouster_hip_cartesian of the filtered
     *     plane bit for bit) in the sensor / body frame; invalid != 0, or a world-frame cloud (xyz_world_frame), throws
     *     std::invalid_argument;
     *   - the per-column gate counts dewarp() reuses are dropped whenever RANGE is modified.
     *  `invalid` is checked against every target's type before anything is launched.
     *  @throw std::invalid_argument with the reference's messages for bad bounds / coord_2d / mask shapes */
    void clip(const std::vector<std::string>& fields, double lower, double upper, double invalid = 0);
    /** @throw std::out_of_range if the batch does not hold the staggered plane of `field` */
    void filter_field(const std::string& field, double lower, double upper, double invalid = 0,
                      const std::vector<std::string>* filtered_fields = nullptr);
    void filter_uv(const std::string& coord_2d, size_t lower, size_t upper, double invalid = 0,
                   const std::vector<std::string>* filtered_fields = nullptr);
    /** One (h, w) mask per sensor (host memory; copied before the call returns); frame f uses masks[f % sensors].
     *  @throw std::invalid_argument when the count is not the sensor count or a mask has another shape */
    void mask(const std::vector<std::string>& fields, const std::vector<core::ImgRef<const uint8_t>>& masks);
    /** Pixels whose `axis` coordinate in the batch's OWN cloud (the stored value, cast to double) lies inside [lower, upper]
     *  are invalidated; second-return fields follow RANGE2's cloud where the batch has one, the others RANGE's.  Needs
     *  BatchOptions::xyz; world_frame must equal BatchOptions::xyz_world_frame (@throw std::invalid_argument otherwise). */
    void filter_xyz(int axis, double lower, double upper, double invalid = 0,
                    const std::vector<std::string>* filtered_fields = nullptr, bool world_frame = false);

    /** algorithm::normals (algorithm/normals.h; csrc/k_normals.hip) of every frame of the decoded batch without leaving HBM: the
     *  staggered RANGE (RANGE2) planes and clouds are read through the shifts the batch destaggers with -- the FIRST sensor's
     *  pixel_shift_by_row, as for frame_ops above -- so no destaggered copy of a cloud is made.  Sensor origins follow the frame
     *  the cloud is in: zeros for a sensor-frame batch (use_extrinsics == false), the translation of the frame's sensor's
     *  sensor_to_body for a body-frame batch, and per column the translation of pose[v] * sensor_to_body from poses_device() for
     *  a world-frame batch (xyz_world_frame); frame f belongs to sensor f % sensors.  The result, double [n_frames][h * w][3]
     *  per return, is owned by the batch (allocated on the first call) and equals the float64 restatement of the reference
     *  (tests/normals_model.py) on the batch's own cloud, ranges and poses, bit for bit.  On the batch's stream; synchronous
     *  (the subtent round trip of ouster_hip_normals).  hip::FrameStream and hip::ShardedBatch have no normals yet.
     *  @throw std::invalid_argument when the batch lacks BatchOptions::xyz or the RANGE plane (dual_return: RANGE2 and its cloud)
     *  @throw std::runtime_error with the reference's messages for non-positive parameters */
    void normals(const NormalsOptions& options = NormalsOptions());
    /** Result of the last normals(): return_index 0 / 1; nullptr before the first call (1: before the first dual call). */
    double* normals_device(int return_index);
    /** One frame's normals of the last normals() (h * w x 3 doubles, in the layout that call chose; synchronous).
     *  @throw std::invalid_argument before normals() has made that return's normals */
    void download_normals(int return_index, uint32_t frame, double* host);

    /** core::voxel_downsample_3d (core/voxel_hash_map.h; csrc/k_voxel.hip) over the result of the last dewarp(): the world-frame
     *  points of all frames form one cloud (a float batch's points are widened, which is exact).  The rows, double (M, 3) in
     *  first-seen order, stay in HBM (voxels_device(), voxel_count()) and equal tests/voxel_model.py on download_dewarped()'s
     *  points bit for bit.  Synchronous, on the batch's context.  Returns M.
     *  @throw std::invalid_argument before the first dewarp(), and with the reference's messages for the parameters and
     *         "voxel_downsample: point outside the int32 voxel grid"
     *  @throw std::runtime_error for FIRST_N_POINT / RANDOM with max_points_per_voxel > 1 (host code only) */
    uint64_t voxel_downsample(double voxel_size, const VoxelOptions& options = VoxelOptions());
    /** algorithm::voxel_downsample_with_normals (algorithm/voxel_downsample.h) over xyz_device(return_index) and the
     *  normals_device(return_index) of a previous normals() made with NormalsOptions::staggered_output, so that normal i belongs to
     *  point i.  Pixels without range have a zero normal and take no part.  Results as above, with voxel_normals_device().
     *  @throw std::invalid_argument when normals() has not made that return's normals, or made them in the destaggered layout */
    uint64_t voxel_downsample_with_normals(double voxel_size, int return_index = 0);
    /** Rows of the last voxel_downsample() / voxel_downsample_with_normals(): double [voxel_count()][3]; nullptr before the first
     *  call and after a call that threw (it leaves no result: voxel_count() is 0 and download_voxels throws). */
    double* voxels_device();
    /** Unit normals of the last voxel_downsample_with_normals(); nullptr when the last call was voxel_downsample(). */
    double* voxel_normals_device();
    uint64_t voxel_count() const { return vox_count_; }
    /** Copy the rows to the host (voxel_count() x 3 doubles each; null pointers are skipped; synchronous).
     *  @throw std::invalid_argument before the first call, or for normals when the last call made none */
    void download_voxels(double* points, double* normals);

    /** ICP (algorithm/align_clouds.h; csrc/k_icp.hip) of the rows of the last voxel_downsample*() -- the source -- against a target
     *  cloud in HBM: the scan-to-scan or scan-to-map step on resident data.  Point to plane when voxel_normals_device() is not null
     *  and target normals are given, point to point otherwise.  The result equals ouster_hip_icp_align on the same arrays bit for
     *  bit.  Synchronous, on the batch's context.
     *  @param target_points_device double [n_target][3]
     *  @param target_normals_device double [n_target][3] or nullptr
     *  @param initial_guess16 row-major 4x4, or nullptr for the identity
     *  @throw std::runtime_error before the first voxel_downsample*(), and for HIP failures
     *  @throw std::invalid_argument with the reference's messages for the parameters and "point_to_point_align: target point
     *         outside the int32 cell grid" (point_to_plane_align: on that route) */
    AlignResult align_voxels(const double* target_points_device, const double* target_normals_device, uint64_t n_target,
                             const double* initial_guess16, const AlignOptions& options = AlignOptions());
    /** The rows of the last voxel_downsample*() as a resident algorithm::IcpTarget (a project extension, algorithm/align_clouds.h):
     *  the keyframe or map later batches align against.  With normals when that call produced them.  The target copies what it
     *  needs and shares ownership of the batch's context, so it may outlive the batch.  options.max_corr_dist is the target's;
     *  synchronous, on the batch's context.
     *  @throw std::runtime_error before the first voxel_downsample*(); std::invalid_argument as IcpTarget's constructors */
    algorithm::IcpTarget make_icp_target(const AlignOptions& options = AlignOptions());
    /** align_voxels against a resident target: no grid work.  Point to plane when the target has normals (the batch's voxel normals
     *  are then required), point to point otherwise; max_corr_dist is the target's.  The result equals the overload above on the
     *  target's arrays bit for bit.  The target may come from another batch or from host arrays: the call runs on the target's
     *  context, on the GPU both must share.
     *  @throw std::runtime_error before the first voxel_downsample*()
     *  @throw std::invalid_argument "DeviceFrameBatch::align_voxels: the target lives on another device"
     *  @throw std::invalid_argument "icp_target: source 0 has no normals and the target has them" and the messages above */
    AlignResult align_voxels(const algorithm::IcpTarget& target, const double* initial_guess16, const AlignOptions& options = AlignOptions());

    /** The scan-to-map steps on resident data (core/voxel_hash_map.h; csrc/k_voxel_map.hip): the rows of the last
     *  voxel_downsample*() go into a resident core::VoxelHashMap3d without leaving HBM.  add_voxels_to is map.add_points(rows),
     *  update_voxel_map is map.update(rows, position3); both equal tests/voxel_map_model.py on download_voxels()'s rows.  The calls
     *  run on the map's context, on the GPU both must share, and are synchronous.
     *  @throw std::runtime_error before the first voxel_downsample*()
     *  @throw std::invalid_argument "DeviceFrameBatch: the map lives on another device" (a host map lives on none), and the map's own */
    void add_voxels_to(core::VoxelHashMap3d& map);
    void update_voxel_map(core::VoxelHashMap3d& map, const double* position3);
    /** map.get_closest_neighbors over the same rows: one neighbour and one squared distance per voxel row stay in HBM
     *  (map_neighbors_device(): double [voxel_count()][3]; map_neighbor_dist_device(): double [voxel_count()]); a row without a
     *  neighbour below max_distance_sq has (0, 0, 0) and max_distance_sq.  Throws as above. */
    void closest_in(const core::VoxelHashMap3d& map, double max_distance_sq = DBL_MAX);
    /** nullptr before the first closest_in() and after a voxel_downsample*() since */
    double* map_neighbors_device();
    double* map_neighbor_dist_device();
    /** Copy them to the host (voxel_count() x 3 and voxel_count() doubles; null pointers are skipped; synchronous).
     *  @throw std::invalid_argument before closest_in() */
    void download_map_neighbors(double* points, double* dist_sq);
    /** registration.align_points_to_map over the rows of the last voxel_downsample*(), which stay in HBM (mapping/icp_registration.h;
     *  csrc/k_registration.hip): bit-identical to ouster_hip_registration_align on download_voxels()'s rows.  Throws as above, and
     *  what the registration refuses (std::invalid_argument). */
    core::Matrix4dR align_voxels_to_map(const core::VoxelHashMap3d& map, const mapping::ICPRegistration& registration, double max_distance,
                                        double kernel_scale);

    /** Per-column body_to_world poses of one frame (w x 16 doubles, row-major 4x4 each; identity
     *  until set), the input of dewarp(). */
    void upload_poses(uint32_t frame, const double* poses_w_by_16);
    /** The poses made where the timestamps are: every valid column (status & 1) of every frame gets core::interp_pose of the
     *  known trajectory at its timestamp * 1e-9 s (core/pose_util.h; what the reference's deskew does per frame with
     *  set_column_pose); the other columns keep the pose they have -- identity on a fresh batch.  x_known_s in seconds,
     *  strictly increasing; timestamps outside extrapolate with the first / last pair.  Asynchronous on the batch's stream,
     *  after decode(); one launch for the whole batch, which also writes the float rows dewarp() of a float batch reads: the
     *  next dewarp() / dewarp_async() uses the new poses.  A world-frame batch (BatchOptions::xyz_world_frame) applies poses
     *  inside decode(): clouds already decoded are not rewritten, the new poses hold from the next decode().
     *  @throw std::invalid_argument with the reference's messages (sizes, fewer than two poses, x_known not increasing) */
    void interp_poses(const std::vector<double>& x_known_s, const std::vector<core::mat4d>& poses_known);
    /** Two known poses, any sign of t1 - t0.  @throw std::invalid_argument for |t1 - t0| < epsilon */
    void interp_poses(double t0, const core::mat4d& x0, double t1, const core::mat4d& x1);
    /** One frame's poses (w x 16 doubles; synchronous). */
    void download_poses(uint32_t frame, double* poses_w_by_16);
    /** [n_frames][w][16] doubles; identity until set (allocated on first use). */
    double* poses_device();
    /** Rows 0..2 of the same poses cast to float, [n_frames][w][12]: what dewarp() of a float batch multiplies with.  nullptr
     *  for an xyz_f64 batch (it reads poses_device()). */
    const float* pose_rows_device();
    /** Range-gated, compacting dewarp of the whole decoded batch, on the device
     *  (core::dewarp(FrameSet, luts, min_range, max_range) with provenance, pose_util.h:475-493 /
     *  impl/dewarp_impl.h:86-115): RANGE planes + status + poses -> world-frame points of type
     *  float (or double with xyz_f64), frames concatenated in index order.  Needs the RANGE plane
     *  and options.xyz (for the LUTs).  Synchronous; returns the number of points. */
    uint64_t dewarp(double min_range, double max_range, bool provenance = false);
    /** The same without the wait: the kernels are queued on the batch's stream and the per-frame offsets stay on the device
     *  (`dewarped_offsets_device()`, [n_frames + 1] u64, the last one the total) -- for pipelines that copy them out with
     *  their own stream (hip::FrameStream).  dewarped_frame_offsets() is NOT updated. */
    void dewarp_async(double min_range, double max_range, bool provenance = false);
    uint64_t* dewarped_offsets_device() { return static_cast<uint64_t*>(d_dw_off_.data()); }
    uint32_t* dewarped_frame_idxs_device() { return static_cast<uint32_t*>(d_dw_fi_.data()); }
    uint32_t* dewarped_col_idxs_device() { return static_cast<uint32_t*>(d_dw_ci_.data()); }
    uint64_t* dewarped_timestamps_device() { return static_cast<uint64_t*>(d_dw_ts_.data()); }
    /** Results of the last dewarp(): device pointers and per-frame exclusive offsets [n_frames+1]. */
    void* dewarped_points_device() { return d_dw_pts_.data(); }
    const std::vector<uint64_t>& dewarped_frame_offsets() const { return dw_offsets_; }
    /** Copy the compacted results to the host (null pointers are skipped). */
    void download_dewarped(void* points, uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns);

   private:
    struct FopsTargets;
    void fops_targets_(const std::vector<std::string>* fields, double invalid, FopsTargets& out);
    void fops_invalidate_(const void* pred, FopsTargets& t);
    DeviceBuffer d_masks_;   // mask(): u8 [sensors][h][w]
    std::shared_ptr<Context> ctx_;
    core::PacketFormat pf_;
    uint32_t n_frames_, h_, w_, slots_;
    uint32_t n_sensors_ = 1;
    std::map<std::string, DeviceBuffer> d_images_;   // render_images: float [n_frames][h][w] per field, made on first use
    size_t stride_;
    BatchOptions opt_;
    std::vector<std::pair<std::string, uint32_t>> fields_;
    ::ouster_hip_format* fmt_ = nullptr;
    std::vector<core::XYZLut> luts_;
    std::vector<int32_t> shifts_;
    std::vector<uint32_t> counts_;
    DeviceBuffer d_packets_, d_ts_, d_mid_, d_status_;
    std::map<std::string, DeviceBuffer> d_planes_, d_dst_;
    DeviceBuffer d_xyz_[2];
    int xyz_field_[2] = {-1, -1};
    DeviceBuffer d_gate_;   // u16 [n_frames][8][w] kept counts per column (gate by-product of decode)
    bool gate_valid_ = false;
    DeviceBuffer d_poses_, d_dw_pts_, d_dw_fi_, d_dw_ci_, d_dw_ts_, d_dw_off_;
    DeviceBuffer d_pose_rows_;   // float output: rows 0..2 of the poses cast to float, [n_frames][w][12]
    std::vector<uint64_t> dw_offsets_;
    std::vector<double> sensor_to_body_;   // [sensors][16], row-major
    DeviceBuffer d_normals_[2];            // normals(): f64 [n_frames][h * w][3] per return, made on first use
    bool normals_staggered_[2] = {false, false};   // the layout the last normals() wrote that return in
    DeviceBuffer d_vox_pts_, d_vox_nrm_;   // voxel_downsample*(): f64 [points in][3], the first vox_count_ rows are the result
    uint64_t vox_count_ = 0;
    bool vox_made_ = false, vox_normals_ = false;
    uint64_t voxel_run_(const void* points, const double* normals, uint64_t n, double voxel_size, const VoxelOptions& o);
    DeviceBuffer d_map_nn_, d_map_d2_;     // closest_in(): f64 [vox_count_][3] and [vox_count_]
    bool map_nn_made_ = false;
    void* voxel_map_handle_(const core::VoxelHashMap3d& map, const char* who);
    bool dw_prov_ = false;
};

}  // namespace hip
}  // namespace sdk
}  // namespace ouster
