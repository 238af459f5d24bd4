// k_registration.h -- launch interface of ICPRegistration's pass (k_registration.hip): one kernel that moves, associates and sums,
// and the fold of the chunks' partials into the header the host reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "k_icp.h"
#include "k_voxel_map.h"

namespace ouster_hip_dev {

constexpr int REG_NS = 16;   // OUSTER_HIP_REG_SUMS: SUMS of tests/registration_model.py

// what a pass leaves for the host
struct RegHeader {
    double sums[REG_NS];
    uint64_t count;
};
static_assert(sizeof(RegHeader) == 136, "one read-back");

struct RegPassArgs {
    const void* src;        // the rows this pass loads: the caller's [n][stride] of f32 / f64 (pass 0), or `moved`
    uint64_t stride;
    uint32_t n;
    int32_t apply;          // apply (q, t) to the loaded row first
    double q[4], t[3];      // the previous pass's estimate
    double max_d2;          // max_distance^2
    double k;               // kernel_scale
    double* moved;          // [n][3] workspace: the rows as this pass associated them
    double* partials;       // [chunks][REG_NS]
    uint32_t* counts;       // [chunks]
    RegHeader* hdr;
    // ouster_hip_registration_step only (nullptr otherwise): what the pass found per row
    uint8_t* flags;         // [n]
    double* neighbours;     // [n][3]
    double* dist_sq;        // [n]
    double* terms;          // tests/cpp/registration_lanes.cpp only (nullptr otherwise): [n][REG_NS], what each row added
};

inline uint32_t reg_chunks(uint32_t n) { return icp_chunks(n); }

#ifdef __HIPCC__
// k_reg_pass<float / double> over ceil(n / ICP_CHUNK) workgroups, then k_reg_fold.  from_f32: the element type of a.src.
hipError_t reg_pass_run(const VMapDev& m, const RegPassArgs& a, bool from_f32, hipStream_t st);
#endif

}  // namespace ouster_hip_dev
