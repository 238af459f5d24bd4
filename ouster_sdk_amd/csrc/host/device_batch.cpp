// device_batch.cpp -- see include/ouster/hip/device_batch.h
#include "ouster/hip/device_batch.h"

#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <map>

#include <cstring>
#include <stdexcept>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace hip {

using namespace core;

DeviceFrameBatch::DeviceFrameBatch(const std::vector<SensorInfo>& sensors, uint32_t n_frames,
                                   const BatchOptions& options)
    : ctx_(options.context ? options.context
                           : std::make_shared<Context>(options.device >= 0 ? options.device : current_device())),
      pf_(sensors.at(0)), n_frames_(n_frames), opt_(options) {
    ScopedContext on_my_context(ctx_);
    if (n_frames == 0) throw std::invalid_argument("DeviceFrameBatch: n_frames must be > 0");
    if (!opt_.tuning_cache.empty()) check(ouster_hip_ctx_set_tuning_cache(ctx_->handle(), opt_.tuning_cache.c_str()));
    const SensorInfo& s0 = sensors[0];
    n_sensors_ = static_cast<uint32_t>(sensors.size());
    h_ = s0.format.pixels_per_column;
    w_ = s0.format.columns_per_frame;
    for (const auto& s : sensors)
        if (s.format.pixels_per_column != h_ || s.format.columns_per_frame != w_ ||
            s.format.udp_profile_lidar != s0.format.udp_profile_lidar ||
            s.format.header_type != s0.format.header_type)
            throw std::invalid_argument("DeviceFrameBatch: sensors of one batch must share a data format");
    slots_ = w_ / pf_.columns_per_packet;
    stride_ = (pf_.lidar_packet_size + 15) & ~size_t{15};

    // which planes: requested ones (must exist in the profile) or the frame defaults
    LidarFrameFieldTypes defaults = get_field_types(s0);
    std::vector<std::string> names = opt_.planes;
    if (names.empty())
        for (const auto& ft : defaults) names.push_back(ft.name);
    auto want = [&](const std::string& n) {
        for (const auto& x : names)
            if (x == n) return true;
        for (const auto& x : opt_.destagger)
            if (x == n) return true;
        return opt_.xyz && (n == ChanField::RANGE || n == ChanField::RANGE2);
    };
    std::vector<bool> nan;
    for (auto it = pf_.begin(); it != pf_.end(); ++it) {  // format order, like the batcher
        if (!want(it->first)) continue;
        uint32_t es = 0;
        bool f16 = false;
        for (const auto& ft : defaults)
            if (ft.name == it->first) {
                f16 = ft.element_type == ChanFieldType::FLOAT16;
                es = static_cast<uint32_t>(field_type_size(ft.element_type)) * (f16 ? 3 : 1);
            }
        if (!es) es = static_cast<uint32_t>(field_type_size(it->second.first)) * it->second.second;
        fields_.emplace_back(it->first, es);
        nan.push_back(f16);
    }
    ouster_hip_format_desc d;
    pf_.fill_hip_desc(w_, fields_, nan, d);
    check(ouster_hip_format_create(default_ctx(), &d, &fmt_));

    const size_t npx = static_cast<size_t>(h_) * w_;
    for (size_t i = 0; i < fields_.size(); ++i) {
        const auto& f = fields_[i];
        bool is_plane = opt_.planes.empty();
        for (const auto& x : opt_.planes) is_plane |= x == f.first;
        if (is_plane) d_planes_[f.first].resize(npx * f.second * n_frames_);
        for (const auto& x : opt_.destagger)
            if (x == f.first) d_dst_[f.first].resize(npx * f.second * n_frames_);
        if (opt_.xyz && f.first == ChanField::RANGE) xyz_field_[0] = static_cast<int>(i);
        if (opt_.xyz && f.first == ChanField::RANGE2) xyz_field_[1] = static_cast<int>(i);
    }
    for (const auto& x : opt_.destagger)
        if (!d_dst_.count(x)) throw std::invalid_argument("DeviceFrameBatch: unknown plane '" + x + "'");
    const size_t xes = opt_.xyz_f64 ? 8 : 4;
    for (int k = 0; k < 2; ++k)
        if (xyz_field_[k] >= 0) d_xyz_[k].resize(npx * 3 * xes * n_frames_);
    if (opt_.xyz)
        for (const auto& s : sensors) luts_.emplace_back(s, opt_.use_extrinsics);
    shifts_.assign(s0.format.pixel_shift_by_row.begin(), s0.format.pixel_shift_by_row.end());
    for (const auto& s : sensors) sensor_to_body_.insert(sensor_to_body_.end(), s.sensor_to_body.m, s.sensor_to_body.m + 16);
    if (!opt_.destagger.empty() && shifts_.size() != h_)
        throw std::invalid_argument("image height does not match shifts size");
    d_packets_.resize(static_cast<size_t>(n_frames_) * slots_ * stride_);
    d_ts_.resize(static_cast<size_t>(n_frames_) * w_ * 8);
    d_mid_.resize(static_cast<size_t>(n_frames_) * w_ * 2);
    d_status_.resize(static_cast<size_t>(n_frames_) * w_ * 4);
    counts_.assign(n_frames_, 0);
    if (opt_.auto_placement && n_frames_ >= 64 && !options.context) {   // a shared context's tuner state is not ours to reset
        if (hipMemsetAsync(d_packets_.data(), 0, d_packets_.size(), static_cast<hipStream_t>(ctx_->stream())) != hipSuccess)
            throw std::runtime_error("ouster_hip: hipMemset(packets) failed");
        refine_placement(opt_.placement_draws, nullptr, opt_.placement_ballast_bytes);
        if (opt_.placement_thorough) {
            tune_placement(10, nullptr, size_t{4} << 30);
            refine_placement(opt_.placement_draws, nullptr, opt_.placement_ballast_bytes);
        }
    }
}

DeviceFrameBatch::~DeviceFrameBatch() {
    ScopedContext on_my_context(ctx_);
    if (fmt_) ouster_hip_format_destroy(fmt_);
}

// A packet that arrives twice is merged into its home slot in arrival order: the later copy's valid columns over the earlier's,
// the later packet's header and footer.  That is what the reference ends up with except in one corner (DESIGN.md section 5 (ii):
// a first copy that ends in invalid columns, re-sent whole before any later packet -- the reference's next_valid bookkeeping then
// zeroes the second copy's tail again, the merged slot keeps it); a caller that needs that corner, or arrival-order semantics for
// packets with rewritten ids, hands ouster_hip_decode the buffer in arrival order with packet counts (general mapping).
void DeviceFrameBatch::stage_packet(uint8_t* slot, bool occupied, const uint8_t* pkt) const {
    if (!occupied) {
        std::memcpy(slot, pkt, pf_.lidar_packet_size);
        return;
    }
    const size_t cols_end = pf_.packet_header_size + static_cast<size_t>(pf_.columns_per_packet) * pf_.col_size;
    std::memcpy(slot, pkt, pf_.packet_header_size);
    std::memcpy(slot + cols_end, pkt + cols_end, pf_.lidar_packet_size - cols_end);
    for (uint32_t ic = 0; ic < pf_.columns_per_packet; ++ic) {
        const uint8_t* col = pf_.nth_col(ic, pkt);
        if ((pf_.col_status(col) & 0x01) != 0u && pf_.col_measurement_id(col) < w_)
            std::memcpy(slot + (col - pkt), col, pf_.col_size);
    }
}

void DeviceFrameBatch::upload_frame_packets(uint32_t frame, const std::vector<const uint8_t*>& packets) {
    ScopedContext on_my_context(ctx_);
    if (frame >= n_frames_) throw std::out_of_range("DeviceFrameBatch: frame index");
    // every packet goes to its home slot (a packet sent twice is merged column by column, stage_packet); slots
    // without a packet are zero = invalid columns
    std::vector<uint8_t> staging(static_cast<size_t>(slots_) * stride_, 0);
    std::vector<bool> have(slots_, false);
    for (const uint8_t* pkt : packets) {
        const int p = home_slot(pkt);
        if (p < 0) continue;
        stage_packet(staging.data() + static_cast<size_t>(p) * stride_, have[static_cast<size_t>(p)], pkt);
        have[static_cast<size_t>(p)] = true;
    }
    d_packets_.upload(staging.data(), staging.size(), static_cast<size_t>(frame) * slots_ * stride_);
    counts_[frame] = slots_;
}

void DeviceFrameBatch::decode() {
    ScopedContext on_my_context(ctx_);
    ouster_hip_frame_out out{};
    for (size_t i = 0; i < fields_.size(); ++i) {
        auto p = d_planes_.find(fields_[i].first);
        if (p != d_planes_.end()) out.planes[i] = p->second.data();
        auto q = d_dst_.find(fields_[i].first);
        if (q != d_dst_.end()) out.destaggered[i] = q->second.data();
    }
    out.timestamp = static_cast<uint64_t*>(d_ts_.data());
    out.measurement_id = static_cast<uint16_t*>(d_mid_.data());
    out.status = static_cast<uint32_t*>(d_status_.data());
    out.xyz_dtype = opt_.xyz_f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32;
    std::vector<const ouster_hip_lut*> luts;
    for (int k = 0; k < 2; ++k) {
        out.xyz_field[k] = xyz_field_[k];
        out.xyz[k] = xyz_field_[k] >= 0 ? d_xyz_[k].data() : nullptr;
    }
    for (const auto& l : luts_) luts.push_back(l.device().handle);
    if (opt_.xyz_world_frame && opt_.xyz) {
        if (d_poses_.size() == 0) upload_poses(0, nullptr);   // identity, like a fresh LidarFrame
        out.xyz_poses = static_cast<const double*>(d_poses_.data());
    }
    gate_valid_ = false;
    if (opt_.gate_max_range >= opt_.gate_min_range) {
        int gf = -1;
        for (size_t i = 0; i < fields_.size(); ++i)
            if (fields_[i].first == ChanField::RANGE) gf = static_cast<int>(i);
        int empty = 0;
        check(ouster_hip_range_gate(opt_.gate_min_range, opt_.gate_max_range, &out.gate_min_r, &out.gate_max_r, &empty));
        if (gf >= 0 && !empty) {
            d_gate_.resize(static_cast<size_t>(n_frames_) * OUSTER_HIP_GATE_CHUNKS * w_ * 2);
            out.gate_counts = static_cast<uint16_t*>(d_gate_.data());
            out.gate_field = gf;
            gate_valid_ = true;
        }
    }
    // per-frame packet counts are only news when a frame has not been uploaded (count 0: it decodes as zeros); a batch whose
    // frames are all there says "every slot counts" with a null pointer and spares the call an upload of the counts
    const bool every_frame = std::all_of(counts_.begin(), counts_.end(), [&](uint32_t c) { return c == slots_; });
    check(ouster_hip_decode(default_ctx(), fmt_, static_cast<const uint8_t*>(d_packets_.data()), stride_,
                            slots_, (opt_.all_slots || every_frame) ? nullptr : counts_.data(), n_frames_, nullptr, &out,
                            d_dst_.empty() ? nullptr : shifts_.data(), luts.empty() ? nullptr : luts.data(),
                            static_cast<uint32_t>(luts.size())));
}

// ---- frame_ops on the resident batch ------------------------------------------------------------------------------------
struct DeviceFrameBatch::FopsTargets {
    std::vector<ouster_hip_fops_plane> planes;   // the staggered planes with their destaggered twins ...
    std::vector<ouster_hip_fops_plane> clouds;   // ... and the clouds of the range planes among them
    std::vector<std::string> names;              // planes[i] is the plane of names[i]
    bool range = false;
};

void DeviceFrameBatch::fops_targets_(const std::vector<std::string>* fields, double invalid, FopsTargets& out) {
    std::vector<std::string> names;
    if (fields) {   // nullptr: every plane (clip / mask hand an empty list over as nullptr, like the reference)
        names = *fields;
    } else {
        for (const auto& f : fields_) names.push_back(f.first);
    }
    for (const auto& name : names) {
        auto p = d_planes_.find(name);
        if (p == d_planes_.end()) continue;
        uint32_t es = 0;
        size_t idx = 0;
        for (size_t i = 0; i < fields_.size(); ++i)
            if (fields_[i].first == name) es = fields_[i].second, idx = i;
        int type = 0;
        switch (es) {
            case 1: type = OUSTER_HIP_U8; break;
            case 2: type = OUSTER_HIP_U16; break;
            case 4: type = OUSTER_HIP_U32; break;
            case 8: type = OUSTER_HIP_U64; break;
            default: continue;   // packed multi-channel planes: not visited, like FLOAT16 in the reference
        }
        uint64_t bits;
        check(ouster_hip_frame_ops_invalid_bits(type, invalid, &bits));
        ouster_hip_fops_plane pl{};
        pl.data = p->second.data();
        auto q = d_dst_.find(name);
        if (q != d_dst_.end()) pl.twin = q->second.data();
        pl.type = type;
        pl.invalid = invalid;
        out.planes.push_back(pl);
        out.names.push_back(name);
        for (int k = 0; k < 2; ++k) {
            if (xyz_field_[k] != static_cast<int>(idx) || d_xyz_[k].size() == 0) continue;
            if (invalid != 0)
                throw std::invalid_argument("DeviceFrameBatch: invalid == " + std::to_string(invalid) + " on " + name +
                                            " of a batch with XYZ is not supported (only 0 is)");
            if (opt_.xyz_world_frame)
                throw std::invalid_argument("DeviceFrameBatch: " + name + " of a batch with world-frame XYZ cannot be a frame_ops target");
            ouster_hip_fops_plane c{};
            c.data = d_xyz_[k].data();
            c.type = opt_.xyz_f64 ? OUSTER_HIP_FOPS_XYZ_F64 : OUSTER_HIP_FOPS_XYZ_F32;
            out.clouds.push_back(c);
        }
        if (name == ChanField::RANGE) out.range = true;
    }
}

void DeviceFrameBatch::fops_invalidate_(const void* pred_in, FopsTargets& t) {
    if (t.planes.empty()) return;
    ouster_hip_fops_pred pred = *static_cast<const ouster_hip_fops_pred*>(pred_in);
    bool twins = false;
    for (const auto& p : t.planes) twins = twins || p.twin != nullptr;
    if (twins || pred.kind == OUSTER_HIP_FOPS_PRED_COLS) {
        if (shifts_.size() != h_) throw std::invalid_argument("image height does not match shifts size");
        pred.shifts = shifts_.data();
        pred.n_shift_tables = 1;
    }
    std::vector<ouster_hip_fops_plane> all = t.planes;
    all.insert(all.end(), t.clouds.begin(), t.clouds.end());
    if (t.range) gate_valid_ = false;   // dewarp() counts again
    check(ouster_hip_frame_ops_invalidate(default_ctx(), &pred, all.data(), static_cast<uint32_t>(all.size()), n_frames_, h_, w_));
}

void DeviceFrameBatch::clip(const std::vector<std::string>& fields, double lower, double upper, double invalid) {
    ScopedContext on_my_context(ctx_);
    FopsTargets t;
    fops_targets_(fields.empty() ? nullptr : &fields, invalid, t);
    if (t.planes.empty()) return;
    // clip is element-wise: the destaggered copy is clipped as a plane of its own, in the same launch
    std::vector<ouster_hip_fops_plane> all;
    for (const auto& p : t.planes) {
        ouster_hip_fops_plane a = p;
        a.twin = nullptr;
        all.push_back(a);
        if (p.twin) {
            a.data = p.twin;
            all.push_back(a);
        }
    }
    if (t.range) gate_valid_ = false;
    check(ouster_hip_frame_ops_clip(default_ctx(), all.data(), static_cast<uint32_t>(all.size()), n_frames_, h_, w_, lower, upper));
    // invalid is 0 here (fops_targets_): a point whose range is now 0 -- clipped, or 0 before, whose point is (0, 0, 0) already --
    // becomes (0, 0, 0)
    size_t c = 0;
    for (size_t i = 0; i < t.planes.size() && c < t.clouds.size(); ++i) {
        if (t.names[i] != ChanField::RANGE && t.names[i] != ChanField::RANGE2) continue;
        ouster_hip_fops_pred pred{};
        pred.kind = OUSTER_HIP_FOPS_PRED_KEY;
        pred.src_type = OUSTER_HIP_U32;
        pred.src = t.planes[i].data;
        pred.lower = pred.upper = 0.0;
        check(ouster_hip_frame_ops_invalidate(default_ctx(), &pred, &t.clouds[c++], 1, n_frames_, h_, w_));
    }
}

void DeviceFrameBatch::filter_field(const std::string& field, double lower, double upper, double invalid,
                                    const std::vector<std::string>* filtered_fields) {
    ScopedContext on_my_context(ctx_);
    auto key = d_planes_.find(field);
    if (key == d_planes_.end()) throw std::out_of_range("DeviceFrameBatch: no plane '" + field + "'");
    ouster_hip_fops_pred pred{};
    pred.kind = OUSTER_HIP_FOPS_PRED_KEY;
    switch (plane_bytes_per_frame(field) / (static_cast<size_t>(h_) * w_)) {
        case 1: pred.src_type = OUSTER_HIP_U8; break;
        case 2: pred.src_type = OUSTER_HIP_U16; break;
        case 4: pred.src_type = OUSTER_HIP_U32; break;
        case 8: pred.src_type = OUSTER_HIP_U64; break;
        default: throw std::invalid_argument("filter_field requires a pixel field with shape (h, w) to build a mask");
    }
    pred.src = key->second.data();
    pred.lower = lower;
    pred.upper = upper;
    FopsTargets t;
    fops_targets_(filtered_fields, invalid, t);
    fops_invalidate_(&pred, t);
}

void DeviceFrameBatch::filter_uv(const std::string& coord_2d, size_t lower, size_t upper, double invalid,
                                 const std::vector<std::string>* filtered_fields) {
    ScopedContext on_my_context(ctx_);
    if (coord_2d != "u" && coord_2d != "v")
        throw std::invalid_argument("coord_2d == " + coord_2d + " must be either 'u' or 'v'");
    const size_t coord_size = coord_2d == "u" ? h_ : w_;
    if (lower > coord_size || upper > coord_size)
        throw std::invalid_argument("lower == " + std::to_string(lower) + " and upper == " + std::to_string(upper) +
                                    " must be in the range [0, " + std::to_string(coord_size) + "]");
    if (lower > upper)
        throw std::invalid_argument("lower == " + std::to_string(lower) + " must be less than upper == " + std::to_string(upper));
    ouster_hip_fops_pred pred{};
    pred.kind = coord_2d == "u" ? OUSTER_HIP_FOPS_PRED_ROWS : OUSTER_HIP_FOPS_PRED_COLS;
    pred.lo = static_cast<uint32_t>(lower);
    pred.hi = static_cast<uint32_t>(upper);
    FopsTargets t;
    fops_targets_(filtered_fields, invalid, t);
    fops_invalidate_(&pred, t);
}

void DeviceFrameBatch::mask(const std::vector<std::string>& fields, const std::vector<ImgRef<const uint8_t>>& masks) {
    ScopedContext on_my_context(ctx_);
    if (masks.size() != n_sensors_)
        throw std::invalid_argument("DeviceFrameBatch::mask needs one mask per sensor: got " + std::to_string(masks.size()) +
                                    ", the batch has " + std::to_string(n_sensors_));
    for (const auto& m : masks)
        if (m.rows() != h_ || m.cols() != w_) throw std::invalid_argument("Used mask size doesn't match frame size");
    FopsTargets t;
    fops_targets_(fields.empty() ? nullptr : &fields, 0, t);
    const size_t npx = static_cast<size_t>(h_) * w_;
    std::vector<uint8_t> all(npx * n_sensors_);
    for (size_t s = 0; s < masks.size(); ++s) std::memcpy(all.data() + s * npx, masks[s].data(), npx);
    sync();   // a mask() still in flight reads the buffer this call is about to overwrite
    d_masks_.resize(all.size());
    d_masks_.upload(all.data(), all.size());   // synchronous: `all` may go
    ouster_hip_fops_pred pred{};
    pred.kind = OUSTER_HIP_FOPS_PRED_MASK;
    pred.src = d_masks_.data();
    pred.n_masks = n_sensors_;
    fops_invalidate_(&pred, t);
}

void DeviceFrameBatch::filter_xyz(int axis, double lower, double upper, double invalid,
                                  const std::vector<std::string>* filtered_fields, bool world_frame) {
    ScopedContext on_my_context(ctx_);
    if (axis < 0 || axis > 2) throw std::invalid_argument("axis_idx == " + std::to_string(axis) + " must be in the range [0, 2]");
    if (!opt_.xyz || (d_xyz_[0].size() == 0 && d_xyz_[1].size() == 0))
        throw std::invalid_argument("DeviceFrameBatch::filter_xyz needs BatchOptions::xyz");
    if (world_frame != opt_.xyz_world_frame)
        throw std::invalid_argument(std::string("DeviceFrameBatch::filter_xyz: world_frame must equal BatchOptions::xyz_world_frame (") +
                                    (opt_.xyz_world_frame ? "true)" : "false)"));
    FopsTargets t;
    fops_targets_(filtered_fields, invalid, t);
    // which cloud decides for a field (python/src/ouster/sdk/core/frame_ops.py:128-136)
    FopsTargets group[2];
    size_t cloud = 0;
    for (size_t i = 0; i < t.planes.size(); ++i) {
        const std::string& n = t.names[i];
        const bool second = n == "RANGE2" || n == "SIGNAL2" || n == "REFLECTIVITY2" || n == "FLAGS2";
        int k = second ? 1 : 0;
        if (d_xyz_[k].size() == 0) k = 1 - k;
        group[k].planes.push_back(t.planes[i]);
        group[k].names.push_back(n);
        if (n == ChanField::RANGE) group[k].range = true;
        if ((n == ChanField::RANGE || n == ChanField::RANGE2) && cloud < t.clouds.size()) group[k].clouds.push_back(t.clouds[cloud++]);
    }
    // A launch reads its own cloud before it writes it (per pixel), and never the other launch's: group 0 reads and may zero
    // RANGE's cloud; group 1 reads RANGE2's.  A cloud zeroed by the OTHER group (RANGE2 following RANGE's cloud for lack of
    // its own is impossible: a RANGE2 plane with XYZ has its cloud) is never a predicate source afterwards.
    for (int k = 0; k < 2; ++k) {
        if (group[k].planes.empty()) continue;
        ouster_hip_fops_pred pred{};
        pred.kind = OUSTER_HIP_FOPS_PRED_XYZ;
        pred.src_type = opt_.xyz_f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32;
        pred.src = d_xyz_[k].data();
        pred.axis = static_cast<uint32_t>(axis);
        pred.lower = lower;
        pred.upper = upper;
        fops_invalidate_(&pred, group[k]);
    }
}

void DeviceFrameBatch::sync() { ctx_->sync(); }

double DeviceFrameBatch::tune_placement(int tries, std::vector<double>* all_ms, size_t ballast_bytes) {
    ScopedContext on_my_context(ctx_);
    auto st = static_cast<hipStream_t>(ctx_->stream());
    struct Events {   // released on every way out, decode() may throw
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } ev;
    if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess)
        throw std::runtime_error("ouster_hip: hipEventCreate failed");
    hipEvent_t e0 = ev.a, e1 = ev.b;
    const std::vector<uint32_t> kept_counts = counts_;
    struct RestoreCounts {   // the caller's per-frame packet counts come back whatever happens
        std::vector<uint32_t>& dst;
        const std::vector<uint32_t>& src;
        ~RestoreCounts() { dst = src; }
    } restore{counts_, kept_counts};
    counts_.assign(n_frames_, slots_);   // time the full-frame work whatever has been uploaded so far
    auto clock = [&]() {
        constexpr int launches = 12;
        decode();
        decode();
        (void)hipEventRecord(e0, st);
        for (int i = 0; i < launches; ++i) decode();
        (void)hipEventRecord(e1, st);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        return static_cast<double>(ms) / launches;
    };
    struct Outputs {
        std::map<std::string, DeviceBuffer> planes, dst;
        DeviceBuffer xyz[2], ts, mid, status;
    };
    auto fresh = [&]() {
        Outputs o;
        for (const auto& kv : d_planes_) o.planes[kv.first].resize(kv.second.size());
        for (const auto& kv : d_dst_) o.dst[kv.first].resize(kv.second.size());
        for (int k = 0; k < 2; ++k)
            if (d_xyz_[k].size()) o.xyz[k].resize(d_xyz_[k].size());
        o.ts.resize(d_ts_.size());
        o.mid.resize(d_mid_.size());
        o.status.resize(d_status_.size());
        return o;
    };
    auto exchange = [&](Outputs& o) {
        std::swap(o.planes, d_planes_);
        std::swap(o.dst, d_dst_);
        for (int k = 0; k < 2; ++k) std::swap(o.xyz[k], d_xyz_[k]);
        std::swap(o.ts, d_ts_);
        std::swap(o.mid, d_mid_);
        std::swap(o.status, d_status_);
    };
    for (int i = 0; i < 16; ++i) decode();   // let the library's variant tuner settle first
    double best = clock();
    if (all_ms) all_ms->push_back(best);
    // the rejected draws stay allocated until the search is over: memory that has just been freed is what the
    // next allocation of the same size gets back, and it would be the same draw again
    std::vector<Outputs> rejected;
    std::vector<DeviceBuffer> rejected_packets;
    for (int t = 1; t < tries; ++t) {
        Outputs cand;
        try {
            cand = fresh();
        } catch (const std::exception&) {   // out of device memory: choose among the draws made so far
            (void)hipGetLastError();        // ... and do not leave the failed hipMalloc behind as the runtime's last error
            break;
        }
        exchange(cand);                  // members = candidate, cand = incumbent
        const double ms = clock();
        if (all_ms) all_ms->push_back(ms);
        if (ms < best) best = ms;        // keep the candidate
        else exchange(cand);             // put the incumbent back
        rejected.push_back(std::move(cand));
        if (ballast_bytes) {
            try {
                rejected_packets.emplace_back(ballast_bytes);
            } catch (const std::exception&) {
                (void)hipGetLastError();
                break;
            }
        }
    }
    ctx_->sync();
    rejected_packets.clear();            // the packet buffer looks for its place in what the ballast occupied
    for (int t = 1; t < std::min(tries, 6); ++t) {
        DeviceBuffer cand;
        try {
            cand.resize(d_packets_.size());
        } catch (const std::exception&) {
            break;
        }
        if (hipMemcpyAsync(cand.data(), d_packets_.data(), d_packets_.size(), hipMemcpyDeviceToDevice, st) != hipSuccess)
            throw std::runtime_error("ouster_hip: packet buffer copy failed");
        std::swap(cand, d_packets_);
        const double ms = clock();
        if (all_ms) all_ms->push_back(ms);
        if (ms < best) best = ms;
        else std::swap(cand, d_packets_);
        rejected_packets.push_back(std::move(cand));
    }
    ctx_->sync();
    rejected.clear();
    rejected_packets.clear();
    // the kernel variant was chosen on the first draw: let the tuner look again on the buffers that stay
    check(ouster_hip_ctx_set_knob(default_ctx(), "retune", 1));
    for (int i = 0; i < 24; ++i) decode();
    best = std::min(best, clock());
    return best * 1e-3;
}

double DeviceFrameBatch::refine_placement(int draws, std::vector<double>* all_ms, size_t ballast_bytes) {
    ScopedContext on_my_context(ctx_);
    auto st = static_cast<hipStream_t>(ctx_->stream());
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } ev;
    if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess)
        throw std::runtime_error("ouster_hip: hipEventCreate failed");
    const std::vector<uint32_t> kept_counts = counts_;
    struct RestoreCounts {
        std::vector<uint32_t>& dst;
        const std::vector<uint32_t>& src;
        ~RestoreCounts() { dst = src; }
    } restore{counts_, kept_counts};
    counts_.assign(n_frames_, slots_);   // the full-frame store pattern whatever has been uploaded so far
    auto clock = [&]() {
        constexpr int launches = 10;
        decode();
        decode();
        (void)hipEventRecord(ev.a, st);
        for (int i = 0; i < launches; ++i) decode();
        (void)hipEventRecord(ev.b, st);
        (void)hipEventSynchronize(ev.b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev.a, ev.b);
        return static_cast<double>(ms) / launches;
    };
    // the groups, heaviest first: pointers to the batch's own buffers
    std::vector<std::vector<DeviceBuffer*>> groups(4);
    for (int k = 0; k < 2; ++k)
        if (d_xyz_[k].size()) groups[0].push_back(&d_xyz_[k]);
    auto elem_of = [&](const std::string& name) {
        for (const auto& f : fields_)
            if (f.first == name) return f.second;
        return 0u;
    };
    for (auto& kv : d_planes_) groups[elem_of(kv.first) >= 4 ? 1 : 3].push_back(&kv.second);
    for (auto& kv : d_dst_) groups[2].push_back(&kv.second);
    // draws - 1 further copies of the whole output set, `ballast_bytes` of device memory apart: copies[c][g][i]
    std::vector<std::vector<std::vector<DeviceBuffer>>> copies;
    std::vector<DeviceBuffer> ballast;
    size_t set_bytes = 0;
    for (const auto& grp : groups)
        for (const DeviceBuffer* b : grp) set_bytes += b->size();
    for (int d = 1; d < draws; ++d) {
        // never take the device to its last byte: a draw needs its copy of the output set plus the ballast, and a quarter
        // of what is free stays free for whoever else uses this GPU
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); break; }
        if (set_bytes + ballast_bytes > free_b - free_b / 4) break;
        try {
            if (ballast_bytes) ballast.emplace_back(ballast_bytes);
            std::vector<std::vector<DeviceBuffer>> set(groups.size());
            for (size_t g = 0; g < groups.size(); ++g) {
                set[g].resize(groups[g].size());
                for (size_t i = 0; i < groups[g].size(); ++i) set[g][i].resize(groups[g][i]->size());
            }
            copies.push_back(std::move(set));
        } catch (const std::exception&) {
            (void)hipGetLastError();   // the failed hipMalloc must not surface as the next launch's error
            break;   // out of device memory: decide among what has been drawn
        }
    }
    for (int i = 0; i < 24; ++i) decode();   // the library's variant tuner settles first
    double best = clock();
    if (all_ms) all_ms->push_back(best);
    for (size_t g = 0; g < groups.size(); ++g) {
        if (groups[g].empty()) continue;
        for (auto& set : copies) {
            for (size_t i = 0; i < groups[g].size(); ++i) std::swap(set[g][i], *groups[g][i]);   // members = this location
            const double ms = clock();
            if (all_ms) all_ms->push_back(ms);
            if (ms < best) best = ms;                                                            // keep it (the incumbent moves into the copy)
            else for (size_t i = 0; i < groups[g].size(); ++i) std::swap(set[g][i], *groups[g][i]);
        }
    }
    ctx_->sync();
    copies.clear();
    ballast.clear();
    check(ouster_hip_ctx_set_knob(default_ctx(), "retune", 1));
    for (int i = 0; i < 24; ++i) decode();
    ctx_->sync();
    return best * 1e-3;
}

size_t DeviceFrameBatch::plane_bytes_per_frame(const std::string& name) const {
    for (const auto& f : fields_)
        if (f.first == name) return static_cast<size_t>(h_) * w_ * f.second;
    throw std::out_of_range("DeviceFrameBatch: unknown plane '" + name + "'");
}

void* DeviceFrameBatch::plane_device(const std::string& name) { return d_planes_.at(name).data(); }
void* DeviceFrameBatch::destaggered_device(const std::string& name) { return d_dst_.at(name).data(); }
void* DeviceFrameBatch::xyz_device(int k) { return d_xyz_[k].data(); }

void DeviceFrameBatch::download_plane(const std::string& name, uint32_t frame, void* host, bool destaggered) {
    ScopedContext on_my_context(ctx_);
    DeviceBuffer& b = destaggered ? d_dst_.at(name) : d_planes_.at(name);
    const size_t bytes = b.size() / n_frames_;
    sync();
    b.download(host, bytes, bytes * frame);
}
void DeviceFrameBatch::download_xyz(int k, uint32_t frame, void* host) {
    ScopedContext on_my_context(ctx_);
    const size_t bytes = d_xyz_[k].size() / n_frames_;
    sync();
    d_xyz_[k].download(host, bytes, bytes * frame);
}
void DeviceFrameBatch::download_headers(uint32_t frame, uint64_t* ts, uint16_t* mid, uint32_t* st) {
    ScopedContext on_my_context(ctx_);
    sync();
    if (ts) d_ts_.download(ts, static_cast<size_t>(w_) * 8, static_cast<size_t>(frame) * w_ * 8);
    if (mid) d_mid_.download(mid, static_cast<size_t>(w_) * 2, static_cast<size_t>(frame) * w_ * 2);
    if (st) d_status_.download(st, static_cast<size_t>(w_) * 4, static_cast<size_t>(frame) * w_ * 4);
}

void* DeviceFrameBatch::render_images(const std::string& field, ImagePipeline& pipe, bool update_state) {
    ScopedContext on_my_context(ctx_);
    const auto it = d_dst_.find(field);
    if (it == d_dst_.end())
        throw std::invalid_argument("DeviceFrameBatch::render_images: the destaggered plane of '" + field +
                                    "' was not requested in BatchOptions::destagger");
    if (pipe.auto_exposure.size() != n_sensors_ || (!pipe.beam_uniformity.empty() && pipe.beam_uniformity.size() != n_sensors_))
        throw std::invalid_argument("DeviceFrameBatch::render_images: the pipeline needs one object per sensor");
    const size_t npx = static_cast<size_t>(h_) * w_, es = plane_bytes_per_frame(field) / npx;
    ChanFieldType type;
    switch (es) {
        case 1: type = ChanFieldType::UINT8; break;
        case 2: type = ChanFieldType::UINT16; break;
        case 4: type = ChanFieldType::UINT32; break;
        default: throw std::invalid_argument("DeviceFrameBatch::render_images: '" + field + "' is not an 8, 16 or 32 bit plane");
    }
    DeviceBuffer& img = d_images_[field];
    if (img.size() != npx * 4 * n_frames_) img.resize(npx * 4 * n_frames_);
    const size_t stride = npx * n_sensors_;   // a sensor's frames are n_sensors_ images apart
    for (uint32_t s = 0; s < n_sensors_ && s < n_frames_; ++s) {
        const uint32_t cnt = (n_frames_ - s + n_sensors_ - 1) / n_sensors_;
        const uint8_t* in = static_cast<const uint8_t*>(it->second.data()) + s * npx * es;
        float* out = static_cast<float*>(img.data()) + s * npx;
        if (pipe.beam_uniformity.empty())
            pipe.auto_exposure[s].update_batch<float>(*ctx_, in, type, cnt, h_, w_, out, update_state, stride, stride);
        else
            pipe.beam_uniformity[s].update_batch<float>(*ctx_, in, type, cnt, h_, w_, out, update_state, &pipe.auto_exposure[s],
                                                        stride, stride);
    }
    return img.data();
}

void DeviceFrameBatch::download_image(const std::string& field, uint32_t frame, float* host) {
    ScopedContext on_my_context(ctx_);
    if (frame >= n_frames_) throw std::out_of_range("DeviceFrameBatch: frame index");
    const auto it = d_images_.find(field);
    if (it == d_images_.end()) throw std::invalid_argument("DeviceFrameBatch::download_image: render_images('" + field + "') first");
    const size_t bytes = static_cast<size_t>(h_) * w_ * 4;
    sync();
    it->second.download(host, bytes, bytes * frame);
}

void DeviceFrameBatch::normals(const NormalsOptions& o) {
    ScopedContext on_my_context(ctx_);
    const int n_ret = o.dual_return ? 2 : 1;
    const std::string range_names[2] = {ChanField::RANGE, ChanField::RANGE2};
    const void* range[2] = {nullptr, nullptr};
    for (int k = 0; k < n_ret; ++k) {
        const auto it = d_planes_.find(range_names[k]);
        if (!opt_.xyz || xyz_field_[k] < 0 || it == d_planes_.end())
            throw std::invalid_argument("DeviceFrameBatch::normals: the batch needs BatchOptions::xyz and the staggered plane of '" +
                                        range_names[k] + "'");
        range[k] = it->second.data();
    }
    if (shifts_.size() != h_) throw std::invalid_argument("image height does not match shifts size");
    const size_t npx = static_cast<size_t>(h_) * w_;
    ouster_hip_normals_desc d{};
    d.xyz = d_xyz_[0].data();
    d.range = static_cast<const uint32_t*>(range[0]);
    d.xyz_rows = npx;
    if (o.dual_return) {
        d.xyz2 = d_xyz_[1].data();
        d.range2 = static_cast<const uint32_t*>(range[1]);
        d.xyz2_rows = npx, d.range2_h = h_, d.range2_w = w_;
    }
    d.n_frames = n_frames_, d.h = h_, d.w = w_;
    d.pixel_shift_by_row = shifts_.data();
    d.staggered_output = o.staggered_output ? 1 : 0;
    d.xyz_dtype = opt_.xyz_f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32;
    d.pixel_search_range = o.pixel_search_range;
    d.min_angle_of_incidence_rad = o.min_angle_of_incidence_rad;
    d.target_distance_m = o.target_distance_m;
    if (opt_.xyz_world_frame) d.poses = poses_device();
    if (opt_.use_extrinsics) {   // without it the cloud is the sensor's own: zeros, or the poses' translations
        d.sensor_to_body = sensor_to_body_.data();
        d.n_sensor_to_body = n_sensors_;
    }
    // refused before anything is allocated
    ouster_hip_normals_consts unused;
    if (ouster_hip_normals_constants(w_, h_, d.min_angle_of_incidence_rad, d.target_distance_m, 0, 0.0, 0, &unused) != OUSTER_HIP_OK)
        throw std::runtime_error(ouster_hip_last_error());
    for (int k = 0; k < n_ret; ++k)
        if (d_normals_[k].size() != npx * 24 * n_frames_) d_normals_[k].resize(npx * 24 * n_frames_);
    d.normals = static_cast<double*>(d_normals_[0].data());
    if (o.dual_return) d.normals2 = static_cast<double*>(d_normals_[1].data());
    if (ouster_hip_normals(default_ctx(), &d) != OUSTER_HIP_OK) throw std::runtime_error(ouster_hip_last_error());
    for (int k = 0; k < n_ret; ++k) normals_staggered_[k] = o.staggered_output;
}

uint64_t DeviceFrameBatch::voxel_run_(const void* points, const double* normals, uint64_t n, double voxel_size, const VoxelOptions& o) {
    ouster_hip_voxel_desc d{};
    d.points = points, d.normals = normals;
    d.n = n, d.out_capacity = n, d.cols = 3;
    d.dtype = opt_.xyz_f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32;
    d.voxel_size = voxel_size;
    d.max_points_per_voxel = o.max_points_per_voxel, d.min_pts_threshold = o.min_pts_threshold;
    d.strategy = static_cast<int32_t>(o.strategy);
    // a call that throws leaves no result: the earlier one is given up before the buffers may move
    vox_count_ = 0;
    vox_made_ = vox_normals_ = map_nn_made_ = false;
    if (!normals && o.strategy != core::VoxelDownsampleStrategy::AVERAGE_POINT && o.max_points_per_voxel > 1)
        throw std::runtime_error("DeviceFrameBatch::voxel_downsample: FIRST_N_POINT / RANDOM with max_points_per_voxel > 1 are "
                                 "sequential host code (core::voxel_downsample_3d on downloaded points)");
    uint64_t n_out = 0;
    if (n) {
        if (d_vox_pts_.size() < n * 24) d_vox_pts_.resize(n * 24);
        if (normals && d_vox_nrm_.size() < n * 24) d_vox_nrm_.resize(n * 24);
        d.out = static_cast<double*>(d_vox_pts_.data());
        d.out_normals = normals ? static_cast<double*>(d_vox_nrm_.data()) : nullptr;
    }
    // n == 0 goes through the call as well: it returns no rows before it looks at anything else, as the reference does
    const int rc = ouster_hip_voxel_downsample(default_ctx(), &d, &n_out);
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    if (rc != OUSTER_HIP_OK) throw std::runtime_error(ouster_hip_last_error());
    vox_count_ = n_out;
    vox_made_ = true, vox_normals_ = normals != nullptr;
    return n_out;
}

uint64_t DeviceFrameBatch::voxel_downsample(double voxel_size, const VoxelOptions& o) {
    ScopedContext on_my_context(ctx_);
    if (dw_offsets_.empty()) throw std::invalid_argument("DeviceFrameBatch::voxel_downsample: dewarp() first");
    return voxel_run_(d_dw_pts_.data(), nullptr, dw_offsets_.back(), voxel_size, o);
}

uint64_t DeviceFrameBatch::voxel_downsample_with_normals(double voxel_size, int k) {
    ScopedContext on_my_context(ctx_);
    if (!normals_device(k)) throw std::invalid_argument("DeviceFrameBatch::voxel_downsample_with_normals: normals() first");
    if (!normals_staggered_[k])
        throw std::invalid_argument("DeviceFrameBatch::voxel_downsample_with_normals: normals() must run with staggered_output, "
                                    "so that normal i belongs to point i");
    return voxel_run_(d_xyz_[k].data(), normals_device(k), static_cast<uint64_t>(n_frames_) * h_ * w_, voxel_size, VoxelOptions());
}

AlignResult DeviceFrameBatch::align_voxels(const double* target_points_device, const double* target_normals_device, uint64_t n_target,
                                           const double* initial_guess16, const AlignOptions& o) {
    ScopedContext on_my_context(ctx_);
    if (!vox_made_) throw std::runtime_error("DeviceFrameBatch::align_voxels: voxel_downsample() or voxel_downsample_with_normals() first");
    static const double none[3] = {0, 0, 0};   // an empty cloud still needs somewhere to point; it is never read
    AlignResult r;
    r.point_to_plane = vox_normals_ && target_normals_device != nullptr;
    ouster_hip_icp_desc d{};
    d.source_points = vox_count_ ? d_vox_pts_.data() : none;
    d.target_points = n_target ? target_points_device : none;
    d.n_source = vox_count_, d.n_target = n_target;
    if (r.point_to_plane) {
        d.source_normals = vox_count_ ? d_vox_nrm_.data() : none, d.target_normals = target_normals_device;
        d.n_source_normals = vox_count_, d.n_target_normals = n_target;
    }
    d.dtype = OUSTER_HIP_F64;
    if (initial_guess16) std::memcpy(d.initial_guess, initial_guess16, sizeof d.initial_guess);
    else std::memcpy(d.initial_guess, core::mat4d::Identity().data(), sizeof d.initial_guess);
    d.max_corr_dist = o.max_corr_dist, d.max_normal_angle_deg = o.max_normal_angle_deg;
    const int rc = ouster_hip_icp_align(default_ctx(), &d);
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    if (rc != OUSTER_HIP_OK) throw std::runtime_error(ouster_hip_last_error());
    r.pose = core::mat4d::FromRowMajor(d.pose);
    r.iterations = d.iterations, r.correspondences = d.correspondences, r.solved = d.solved != 0;
    return r;
}

algorithm::IcpTarget DeviceFrameBatch::make_icp_target(const AlignOptions& o) {
    ScopedContext on_my_context(ctx_);
    if (!vox_made_) throw std::runtime_error("DeviceFrameBatch::make_icp_target: voxel_downsample() or voxel_downsample_with_normals() first");
    return algorithm::IcpTarget::from_device(static_cast<const double*>(d_vox_pts_.data()),
                                             vox_normals_ ? static_cast<const double*>(d_vox_nrm_.data()) : nullptr, vox_count_, o.max_corr_dist);
}

AlignResult DeviceFrameBatch::align_voxels(const algorithm::IcpTarget& target, const double* initial_guess16, const AlignOptions& o) {
    ScopedContext on_my_context(ctx_);
    if (!vox_made_) throw std::runtime_error("DeviceFrameBatch::align_voxels: voxel_downsample() or voxel_downsample_with_normals() first");
    // the rows stay where they are: a target on another GPU cannot read them.  On the batch's GPU the call runs on the target's own
    // context, whichever that is; the batch's voxel rows are complete (voxel_downsample*() is synchronous)
    if (target.device() >= 0 && target.device() != ctx_->device())
        throw std::invalid_argument("DeviceFrameBatch::align_voxels: the target lives on another device");
    AlignResult r;
    r.point_to_plane = target.has_normals();
    double pose[16];
    const algorithm::impl::AlignStats s =
        target.align_device(static_cast<const double*>(d_vox_pts_.data()),
                            r.point_to_plane && vox_normals_ ? static_cast<const double*>(d_vox_nrm_.data()) : nullptr, vox_count_,
                            initial_guess16, o.max_normal_angle_deg, pose);
    r.pose = core::mat4d::FromRowMajor(pose);
    r.iterations = s.iterations, r.correspondences = s.correspondences, r.solved = s.solved;
    return r;
}

void* DeviceFrameBatch::voxel_map_handle_(const core::VoxelHashMap3d& map, const char* who) {
    if (!vox_made_) throw std::runtime_error(std::string("DeviceFrameBatch::") + who + ": voxel_downsample() or voxel_downsample_with_normals() first");
    // the rows stay where they are: a map on another GPU, or in host memory, cannot read them
    if (map.device() != ctx_->device()) throw std::invalid_argument("DeviceFrameBatch: the map lives on another device");
    if (!map.handle()) throw std::runtime_error("VoxelHashMap3d: moved from");
    return map.handle();
}

namespace {
void raise_map(int rc) {
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    if (rc != OUSTER_HIP_OK) throw std::runtime_error(ouster_hip_last_error());
}
}  // namespace

void DeviceFrameBatch::add_voxels_to(core::VoxelHashMap3d& map) {
    ScopedContext on_my_context(ctx_);
    auto* h = static_cast<ouster_hip_voxel_map*>(voxel_map_handle_(map, "add_voxels_to"));
    raise_map(ouster_hip_voxel_map_add_points(h, d_vox_pts_.data(), OUSTER_HIP_F64, vox_count_, 3));
}

void DeviceFrameBatch::update_voxel_map(core::VoxelHashMap3d& map, const double* position3) {
    ScopedContext on_my_context(ctx_);
    auto* h = static_cast<ouster_hip_voxel_map*>(voxel_map_handle_(map, "update_voxel_map"));
    raise_map(ouster_hip_voxel_map_update(h, d_vox_pts_.data(), OUSTER_HIP_F64, vox_count_, 3, position3));
}

void DeviceFrameBatch::closest_in(const core::VoxelHashMap3d& map, double max_distance_sq) {
    ScopedContext on_my_context(ctx_);
    auto* h = static_cast<ouster_hip_voxel_map*>(voxel_map_handle_(map, "closest_in"));
    map_nn_made_ = false;
    if (vox_count_) {
        if (d_map_nn_.size() < vox_count_ * 24) d_map_nn_.resize(vox_count_ * 24);
        if (d_map_d2_.size() < vox_count_ * 8) d_map_d2_.resize(vox_count_ * 8);
    }
    raise_map(ouster_hip_voxel_map_closest(h, d_vox_pts_.data(), OUSTER_HIP_F64, vox_count_, 3, max_distance_sq,
                                           static_cast<double*>(d_map_nn_.data()), static_cast<double*>(d_map_d2_.data())));
    map_nn_made_ = true;
}

core::Matrix4dR DeviceFrameBatch::align_voxels_to_map(const core::VoxelHashMap3d& map, const mapping::ICPRegistration& registration,
                                                     double max_distance, double kernel_scale) {
    ScopedContext on_my_context(ctx_);
    voxel_map_handle_(map, "align_voxels_to_map");
    return registration.align_device_points_to_map(static_cast<const double*>(d_vox_pts_.data()), vox_count_, 3, map, max_distance, kernel_scale);
}

double* DeviceFrameBatch::map_neighbors_device() { return map_nn_made_ ? static_cast<double*>(d_map_nn_.data()) : nullptr; }
double* DeviceFrameBatch::map_neighbor_dist_device() { return map_nn_made_ ? static_cast<double*>(d_map_d2_.data()) : nullptr; }

void DeviceFrameBatch::download_map_neighbors(double* points, double* dist_sq) {
    ScopedContext on_my_context(ctx_);
    if (!map_nn_made_) throw std::invalid_argument("DeviceFrameBatch::download_map_neighbors: closest_in() first");
    if (!vox_count_) return;
    if (points) d_map_nn_.download(points, vox_count_ * 24);
    if (dist_sq) d_map_d2_.download(dist_sq, vox_count_ * 8);
}

double* DeviceFrameBatch::voxels_device() { return vox_made_ ? static_cast<double*>(d_vox_pts_.data()) : nullptr; }

double* DeviceFrameBatch::voxel_normals_device() {
    return vox_made_ && vox_normals_ ? static_cast<double*>(d_vox_nrm_.data()) : nullptr;
}

void DeviceFrameBatch::download_voxels(double* points, double* normals) {
    ScopedContext on_my_context(ctx_);
    if (!vox_made_) throw std::invalid_argument("DeviceFrameBatch::download_voxels: voxel_downsample() first");
    if (normals && !vox_normals_)
        throw std::invalid_argument("DeviceFrameBatch::download_voxels: the last call was voxel_downsample(), which makes no normals");
    if (!vox_count_) return;
    if (points) d_vox_pts_.download(points, vox_count_ * 24);
    if (normals) d_vox_nrm_.download(normals, vox_count_ * 24);
}

double* DeviceFrameBatch::normals_device(int k) {
    return k >= 0 && k < 2 && d_normals_[k].size() ? static_cast<double*>(d_normals_[k].data()) : nullptr;
}

void DeviceFrameBatch::download_normals(int k, uint32_t frame, double* host) {
    ScopedContext on_my_context(ctx_);
    if (frame >= n_frames_) throw std::out_of_range("DeviceFrameBatch: frame index");
    if (!normals_device(k)) throw std::invalid_argument("DeviceFrameBatch::download_normals: normals() first");
    const size_t bytes = static_cast<size_t>(h_) * w_ * 24;
    sync();
    d_normals_[k].download(host, bytes, bytes * frame);
}

void DeviceFrameBatch::upload_poses(uint32_t frame, const double* poses) {
    ScopedContext on_my_context(ctx_);
    if (frame >= n_frames_) throw std::out_of_range("DeviceFrameBatch: frame index");
    const size_t per = static_cast<size_t>(w_) * 128;
    if (d_poses_.size() == 0) {  // identity for every column, like a fresh LidarFrame
        std::vector<double> ident(static_cast<size_t>(n_frames_) * w_ * 16, 0.0);
        for (size_t i = 0; i < ident.size(); i += 16) ident[i] = ident[i + 5] = ident[i + 10] = ident[i + 15] = 1.0;
        d_poses_.resize(ident.size() * 8);
        d_poses_.upload(ident.data(), ident.size() * 8);
    }
    if (poses) d_poses_.upload(poses, per, per * frame);
    // float output: the range-gated dewarp takes the poses as rows 0..2 cast to float (what dewarp<float> multiplies with,
    // pose_util.h:38-56), converted here on the host: 48 B per column on the device instead of 128
    if (!opt_.xyz_f64) {
        const size_t rows_per = static_cast<size_t>(w_) * 12;
        if (d_pose_rows_.size() == 0) {
            std::vector<float> ident(static_cast<size_t>(n_frames_) * rows_per, 0.0f);
            for (size_t i = 0; i < ident.size(); i += 12) ident[i] = ident[i + 5] = ident[i + 10] = 1.0f;
            d_pose_rows_.resize(ident.size() * 4);
            d_pose_rows_.upload(ident.data(), ident.size() * 4);
        }
        if (poses) {
            std::vector<float> rows(rows_per);
            for (size_t c = 0; c < w_; ++c)
                for (size_t k = 0; k < 12; ++k) rows[c * 12 + k] = static_cast<float>(poses[c * 16 + k]);
            d_pose_rows_.upload(rows.data(), rows_per * 4, rows_per * 4 * frame);
        }
    }
}

const float* DeviceFrameBatch::pose_rows_device() {
    poses_device();
    return opt_.xyz_f64 ? nullptr : static_cast<const float*>(d_pose_rows_.data());
}

double* DeviceFrameBatch::poses_device() {
    if (d_poses_.size() == 0 || (!opt_.xyz_f64 && d_pose_rows_.size() == 0)) upload_poses(0, nullptr);
    return static_cast<double*>(d_poses_.data());
}

void DeviceFrameBatch::interp_poses(const std::vector<double>& x_known, const std::vector<mat4d>& poses_known) {
    ScopedContext on_my_context(ctx_);
    if (x_known.size() != poses_known.size()) throw std::invalid_argument("x_known and poses_known sizes are not matching");
    static_assert(sizeof(mat4d) == 128, "mat4d is 16 packed doubles");
    const uint32_t k = static_cast<uint32_t>(x_known.size());
    const double* known = poses_known.empty() ? nullptr : poses_known[0].m;
    check(ouster_hip_pose_validate(x_known.data(), known, k, nullptr, 0));   // refuses before anything is allocated
    double* poses = poses_device();
    check(ouster_hip_interp_pose_columns(default_ctx(), static_cast<const uint64_t*>(d_ts_.data()),
                                         static_cast<const uint32_t*>(d_status_.data()), n_frames_, w_, x_known.data(), known, k,
                                         poses, opt_.xyz_f64 ? nullptr : static_cast<float*>(d_pose_rows_.data())));
}

void DeviceFrameBatch::interp_poses(double t0, const mat4d& x0, double t1, const mat4d& x1) {
    ScopedContext on_my_context(ctx_);
    if (std::fabs(t1 - t0) < DBL_EPSILON) throw std::invalid_argument("Cannot interpolate with zero duration between poses");
    double* poses = poses_device();
    check(ouster_hip_interp_pose_pair_columns(default_ctx(), static_cast<const uint64_t*>(d_ts_.data()),
                                              static_cast<const uint32_t*>(d_status_.data()), n_frames_, w_, t0, x0.m, t1, x1.m,
                                              poses, opt_.xyz_f64 ? nullptr : static_cast<float*>(d_pose_rows_.data())));
}

void DeviceFrameBatch::download_poses(uint32_t frame, double* poses) {
    ScopedContext on_my_context(ctx_);
    if (frame >= n_frames_) throw std::out_of_range("DeviceFrameBatch: frame index");
    poses_device();
    const size_t per = static_cast<size_t>(w_) * 128;
    sync();
    d_poses_.download(poses, per, per * frame);
}

uint64_t DeviceFrameBatch::dewarp(double min_range, double max_range, bool provenance) {
    dewarp_async(min_range, max_range, provenance);
    ScopedContext on_my_context(ctx_);
    dw_offsets_.resize(static_cast<size_t>(n_frames_) + 1);
    d_dw_off_.download(dw_offsets_.data(), dw_offsets_.size() * 8);  // synchronous
    return dw_offsets_.back();
}

void DeviceFrameBatch::dewarp_async(double min_range, double max_range, bool provenance) {
    ScopedContext on_my_context(ctx_);
    auto rp = d_planes_.find(ChanField::RANGE);
    if (rp == d_planes_.end() || luts_.empty())
        throw std::invalid_argument("DeviceFrameBatch::dewarp needs the RANGE plane and options.xyz");
    if (d_poses_.size() == 0) upload_poses(0, nullptr);
    const size_t cap = static_cast<size_t>(n_frames_) * h_ * w_;
    d_dw_pts_.resize(cap * (opt_.xyz_f64 ? 24 : 12));
    d_dw_off_.resize((static_cast<size_t>(n_frames_) + 1) * 8);
    dw_prov_ = provenance;
    if (provenance) {
        d_dw_fi_.resize(cap * 4);
        d_dw_ci_.resize(cap * 4);
        d_dw_ts_.resize(cap * 8);
    }
    std::vector<const ouster_hip_lut*> luts;
    for (const auto& l : luts_) luts.push_back(l.device().handle);
    // decode() already counted the gated pixels per column when it ran with this very gate
    const bool counted = gate_valid_ && min_range == opt_.gate_min_range && max_range == opt_.gate_max_range;
    if (!opt_.xyz_f64 && d_pose_rows_.size())
        check(ouster_hip_dewarp_frames_rows(
            default_ctx(), luts.data(), static_cast<uint32_t>(luts.size()),
            static_cast<const uint32_t*>(rp->second.data()), static_cast<const uint32_t*>(d_status_.data()),
            static_cast<const uint64_t*>(d_ts_.data()), static_cast<const float*>(d_pose_rows_.data()), n_frames_, min_range,
            max_range, d_dw_pts_.data(), provenance ? static_cast<uint32_t*>(d_dw_fi_.data()) : nullptr,
            provenance ? static_cast<uint32_t*>(d_dw_ci_.data()) : nullptr,
            provenance ? static_cast<uint64_t*>(d_dw_ts_.data()) : nullptr, cap, static_cast<uint64_t*>(d_dw_off_.data()),
            counted ? static_cast<const uint16_t*>(d_gate_.data()) : nullptr));
    else
    check(ouster_hip_dewarp_frames_counted(
        default_ctx(), luts.data(), static_cast<uint32_t>(luts.size()),
        static_cast<const uint32_t*>(rp->second.data()), static_cast<const uint32_t*>(d_status_.data()),
        static_cast<const uint64_t*>(d_ts_.data()), static_cast<const double*>(d_poses_.data()), n_frames_,
        min_range, max_range, opt_.xyz_f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32, d_dw_pts_.data(),
        provenance ? static_cast<uint32_t*>(d_dw_fi_.data()) : nullptr,
        provenance ? static_cast<uint32_t*>(d_dw_ci_.data()) : nullptr,
        provenance ? static_cast<uint64_t*>(d_dw_ts_.data()) : nullptr, cap,
        static_cast<uint64_t*>(d_dw_off_.data()), counted ? static_cast<const uint16_t*>(d_gate_.data()) : nullptr));
}

void DeviceFrameBatch::download_dewarped(void* points, uint32_t* fi, uint32_t* ci, uint64_t* ts) {
    ScopedContext on_my_context(ctx_);
    if (dw_offsets_.empty()) throw std::logic_error("DeviceFrameBatch: dewarp() has not run");
    const size_t n = dw_offsets_.back();
    if (!n) return;
    if (points) d_dw_pts_.download(points, n * (opt_.xyz_f64 ? 24 : 12));
    if ((fi || ci || ts) && !dw_prov_) throw std::logic_error("DeviceFrameBatch: dewarp() ran without provenance");
    if (fi) d_dw_fi_.download(fi, n * 4);
    if (ci) d_dw_ci_.download(ci, n * 4);
    if (ts) d_dw_ts_.download(ts, n * 8);
}

}  // namespace hip
}  // namespace sdk
}  // namespace ouster
