// icp_host.h -- the host half of point_to_point_align / point_to_plane_align (csrc/host/icp_util.cpp): validation with the
// reference's messages, the constants of a call, the two solves behind the sums of a pass, the stop rules, and the plain C++
// restatement behind ouster_hip_icp_align_ref / ouster_hip_icp_step_ref.  Plain C++, no HIP: the C ABI (capi_icp.hip) calls
// it before anything touches the GPU and after each pass's read-back.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

enum IcpMethod : int32_t { ICP_POINT = 0, ICP_PLANE = 1 };

constexpr uint64_t ICP_MIN_POINTS = 20;
constexpr uint32_t ICP_MAX_ITERATIONS = 10;
constexpr uint64_t ICP_MAX_ROWS = 1ull << 30;
constexpr double ICP_NORMAL_EPS = 1e-12;

// nullptr, or what the call is refused with: the reference's four in its order, then the checks of this interface (normals on one
// side only, dtype, strides, NULL pointers)
const char* icp_validate(const ouster_hip_icp_desc* d);
inline IcpMethod icp_method(const ouster_hip_icp_desc* d) { return d->source_normals ? ICP_PLANE : ICP_POINT; }
const char* icp_msg_grid(IcpMethod m);

double icp_cos_gate(double max_normal_angle_deg);
// sigma = 1.4826 mad, replaced by max(1e-3, 0.25 max_corr_dist) where it is not finite or below 1e-4; delta = 1.5 sigma
double icp_huber_delta(double median, double max_corr_dist);

// a = u diag(sigma) v^T by one-sided Jacobi, sigma descending, u's third column the cross product of its first two, signed like
// a's third column; false where
// the second singular value is zero or not finite
bool icp_svd3(const double (&a)[3][3], double (&u)[3][3], double (&sigma)[3], double (&v)[3][3]);
// h x = b by L D L^T without pivoting; false where a pivot is not positive or x not finite
bool icp_ldlt6(const double (&h)[6][6], const double (&b)[6], double (&x)[6]);

// The end of a pass, given its count and sums (OUSTER_HIP_ICP_SUMS) and, point to point, the centroids: next16 = delta * pose16 and
// *stop by the reference's rules; next16 = pose16 and *stop = true where nothing can be solved.
void icp_finish_pass(IcpMethod m, uint64_t count, const double* sums, const double* cx, const double* cq, const double* pose16,
                     double* next16, bool* stop);

// ---- IcpTarget: a resident target and many sources per call (ouster_hip_icp_target_*) ----
constexpr uint32_t ICP_CHUNK_ROWS = 1024;       // k_icp.h: ICP_CHUNK, the rows a workgroup of the sum kernels owns
constexpr uint32_t ICP_MAX_SOURCES = 65535;

// a run of at most ICP_CHUNK_ROWS rows of one source, starting at a multiple of ICP_CHUNK_ROWS of that source's own rows: what
// one workgroup of the many-source kernels owns.  The runs of a source are those of the single call, which is why its sums are.
struct IcpChunk {
    uint32_t source, first, rows;
};

// nullptr, or what ouster_hip_icp_target_create refuses `d` with (the checks after the NULL arguments, in the header's order)
const char* icp_target_validate(const ouster_hip_icp_target_desc* d);
// OUSTER_HIP_OK, or the code ouster_hip_icp_target_align / _step refuse the sources with and the message in msg[cap]: on a plane
// target the angle, then the rows of every source's normals; normals on one side only; dtype, strides, NULL points; the two limits
int icp_sources_validate(bool target_has_normals, const ouster_hip_icp_source* sources, uint32_t n_sources, int32_t dtype,
                         double max_normal_angle_deg, char* msg, size_t cap);
// The chunk table of sources of rows[k] rows (0: the source takes no part and gets no chunk): chunks[] in source order, and per
// source its first row in the concatenated per-row outputs and its first chunk.  Returns the number of chunks; writes at most
// `cap` of them (chunks may be nullptr with cap 0 to count); first_row / first_chunk may be nullptr.
uint64_t icp_chunk_table(const uint64_t* rows, uint32_t n_sources, IcpChunk* chunks, uint64_t cap, uint64_t* first_row,
                         uint64_t* first_chunk);

// the C ABI's error channel (ouster_hip_capi.hip): stores the thread's message, returns `code`
int fail_msg(int code, const char* msg);

}  // namespace ouster_hip_dev
