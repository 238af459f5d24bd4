// tonemap_lanes.cpp -- k_tm_hist, k_tm_luts and k_tm_finish of csrc/k_tonemap.hip compiled for the CPU
// (tests/cpp/host_lanes/hip/hip_runtime.h: one thread per lane, 64 lanes per workgroup) and driven the way ouster_hip_image_tonemap
// drives them.  Built and run by tests/test_tonemap_lanes_cpu.py, which compares the result with tests/tonemap_model.py bit for bit.
//   tonemap_lanes <case file> <result file>
// case file: u32 in_type (12 F16 / 9 F32 / 10 F64), n_images, h, w, in_stride, out_stride (elements), in_place, pieces (0: the
// launch's own choice); n_images ouster_hip_tonemap_params; the input buffer, n_images * in_stride elements; then, unless in place,
// the output buffer as it is before the call, n_images * out_stride elements of T.
// result file: the output buffer, luts f32 [n_images][64][1024], hist u32 [n_images][64][1024].
#include "../../ouster_sdk_amd/csrc/k_tonemap.hip"

#include "host_lanes/lanes_util.h"

using namespace ouster_hip_dev;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t hd[8];
    if (!f || !rd(hd, sizeof hd, f)) return 2;
    const uint32_t in_type = hd[0], n = hd[1], h = hd[2], w = hd[3], in_stride = hd[4], out_stride = hd[5], in_place = hd[6];
    const int out_type = in_type == OUSTER_HIP_F64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32;
    const size_t es_in = in_type == OUSTER_HIP_F16 ? 2 : in_type == OUSTER_HIP_F32 ? 4 : 8, es_out = out_type == OUSTER_HIP_F32 ? 4 : 8;
    if (n == 0 || h < 8 || w < 8 || in_stride < 3 * h * w || out_stride < 3 * h * w || (in_place && (es_in != es_out || in_stride != out_stride))) return 2;
    std::vector<ouster_hip_tonemap_params> params(n);
    // 16-byte aligned buffers, as the device's
    std::vector<double> in_buf((n * in_stride * es_in + 15) / 8 + 2), out_buf(in_place ? 0 : (n * out_stride * es_out + 15) / 8 + 2);
    bool ok = rd(params.data(), n * sizeof params[0], f) && rd(in_buf.data(), n * in_stride * es_in, f);
    if (!in_place) ok = ok && rd(out_buf.data(), n * out_stride * es_out, f);
    std::fclose(f);
    if (!ok) return 2;

    std::vector<uint32_t> hist((size_t)n * TM_LUT_ELEMS, 0);
    std::vector<float> luts((size_t)n * TM_LUT_ELEMS, -7.25f);
    TonemapArgs a{};
    a.in = in_buf.data();
    a.out = in_place ? (void*)in_buf.data() : (void*)out_buf.data();
    a.in_stride = in_stride, a.out_stride = out_stride;
    a.n_images = n, a.h = h, a.w = w;
    const size_t al_in = es_in * 4 < 16 ? es_in * 4 : 16;
    a.vec = n == 1 || ((in_stride * es_in) % al_in == 0 && (out_stride * es_out) % 16 == 0);
    a.params = params.data();
    a.hist = hist.data(), a.luts = luts.data();
    a.pieces = hd[7];
    if (tm_hist_launch<64>(a, (int)in_type, out_type, nullptr) != hipSuccess || tm_luts_launch<64>(a, nullptr) != hipSuccess ||
        tm_finish_launch<64>(a, (int)in_type, out_type, nullptr) != hipSuccess)
        return 3;

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(a.out, 1, n * out_stride * es_out, f);
    std::fwrite(luts.data(), 4, luts.size(), f);
    std::fwrite(hist.data(), 4, hist.size(), f);
    std::fclose(f);
    return 0;
}
