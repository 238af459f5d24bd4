// A reference caller's spelling of the RGB display-image calls, compiled with -DOUSTER_HIP_USE_EIGEN (Eigen and its Tensor module
// mocked by tests/cpp/mock_eigen in this image): Eigen::TensorMap<rgb_img_t<T>> temporaries where the mirror takes RgbImgRef<T>.
// Needs no GPU: it checks the views the conversions give and that argument errors surface through them.  Prints "ok".
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <unsupported/Eigen/CXX11/Tensor>

#include "ouster/core/image_processing.h"

using namespace ouster::sdk::core;
template <typename T> using rgb_img_t = Eigen::Tensor<T, 3, Eigen::RowMajor>;   // the reference's typedefs.h

template <typename F>
static bool refuses(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    } catch (const std::exception&) {
    }
    return false;
}

int main() {
    const int h = 7, w = 16;   // 7 rows: LocalToneMapper refuses the image before it looks for a GPU
    std::vector<float> f(h * w * 3, 0.5f), out(h * w * 3, -7.25f);
    std::vector<double> d(h * w * 3, 0.5);
    std::vector<float16_t> half(h * w * 3);
    // temporaries bind, const and non-const, and the view is the tensor's memory and shape
    RgbImgRef<float> rf = Eigen::TensorMap<rgb_img_t<float>>(f.data(), h, w, 3);
    RgbImgRef<const float16_t> rh = Eigen::TensorMap<const rgb_img_t<float16_t>>(half.data(), h, w, 3);
    RgbImgRef<const double> rd = Eigen::TensorMap<rgb_img_t<double>>(d.data(), h, w, 3);
    rgb_img_t<float> owned(h, w, 3);
    RgbImgRef<float> ro = owned;
    const rgb_img_t<float>& c_owned = owned;
    RgbImgRef<const float> rc = c_owned;
    if (rf.data() != f.data() || rf.rows() != 7 || rf.cols() != 16 || rh.data() != half.data() || rd.data() != d.data() ||
        ro.data() != owned.data() || rc.data() != owned.data() || &rf(2, 3, 1) != f.data() + (2 * 16 + 3) * 3 + 1) {
        std::printf("a view differs from its tensor\n");
        return 1;
    }
    static_assert(!std::is_constructible<RgbImgRef<float>, const rgb_img_t<float>&>::value, "a const tensor gives no mutable view");
    static_assert(!std::is_constructible<RgbImgRef<float>, Eigen::TensorMap<rgb_img_t<double>>>::value, "another scalar gives no view");
    // another channel count or layout is refused
    if (!refuses([&] { RgbImgRef<float> r = Eigen::TensorMap<rgb_img_t<float>>(f.data(), h, w * 3 / 4, 4); (void)r; }) ||
        !refuses([&] { RgbImgRef<float> r = Eigen::TensorMap<Eigen::Tensor<float, 3, Eigen::ColMajor>>(f.data(), h, w, 3); (void)r; })) {
        std::printf("a tensor that is no row-major H x W x 3 image was accepted\n");
        return 2;
    }
    // the reference's calls, exactly as written there
    image::LocalToneMapper tm;
    image::AutoExposure ae;
    if (!refuses([&] { tm.update(Eigen::TensorMap<rgb_img_t<float>>(f.data(), h, w, 3)); }) ||
        !refuses([&] { tm.update(Eigen::TensorMap<rgb_img_t<double>>(d.data(), h, w, 3), false); }) ||
        !refuses([&] { tm.update(Eigen::TensorMap<const rgb_img_t<float16_t>>(half.data(), h, w, 3), Eigen::TensorMap<rgb_img_t<float>>(out.data(), h, w, 3)); }) ||
        !refuses([&] { ae.update(Eigen::TensorMap<const rgb_img_t<float16_t>>(half.data(), h, w, 3), Eigen::TensorMap<rgb_img_t<float>>(out.data(), h, w / 2, 3)); })) {
        std::printf("an argument error did not surface through a TensorMap\n");
        return 3;
    }
    for (float v : out)
        if (v != -7.25f) return 4;
    std::printf("ok\n");
    return 0;
}
