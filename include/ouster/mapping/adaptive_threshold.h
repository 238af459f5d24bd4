/**
 * @file
 * @brief The adaptive correspondence threshold that goes with ICPRegistration.
 *
 * The members, defaults and arithmetic of the reference's ouster/mapping/adaptive_threshold.h.  The arithmetic is plain host code
 * (csrc/host/registration_util.cpp through ouster_hip_registration_model_error) and equals tests/registration_model.py: the
 * rotation angle comes as Eigen's AngleAxisd(R).angle() gives it, matrix to quaternion, then 2 atan2(|vec|, |w|); the rounding order
 * of the norms is the project's ((x x + y y) + z z).
 */
#pragma once

#include <cmath>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"

namespace ouster {
namespace sdk {
namespace mapping {

/// Adaptive threshold for ICP registration.
struct OUSTER_API_CLASS AdaptiveThreshold {
    /// @param[in] max_range Maximum range of the sensor.
    /// @param[in] initial_threshold Initial threshold.
    /// @param[in] min_motion_threshold A deviation counts only strictly above it.
    explicit AdaptiveThreshold(double max_range, double initial_threshold = 2.0, double min_motion_threshold = 0.01)
        : min_motion_threshold_(min_motion_threshold), max_range_(max_range), model_sse_(initial_threshold * initial_threshold), num_samples_(1) {}

    /// Update the belief of the deviation from the prediction model: |t| + 2 max_range sin(theta / 2) of a row-major 4 x 4.
    OUSTER_API_FUNCTION
    void update_model_deviation(const core::mat4d& current_deviation);

    /// The threshold used in registration: sqrt(sse / samples).
    double compute_threshold() const { return std::sqrt(model_sse_ / num_samples_); }

    double min_motion_threshold_;
    double max_range_;
    double model_sse_;
    int num_samples_;
};

}  // namespace mapping
}  // namespace sdk
}  // namespace ouster
