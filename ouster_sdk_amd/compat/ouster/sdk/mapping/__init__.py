"""`ouster.sdk.mapping`: of the reference's mapping package, the frame-to-map registration (ouster_mapping/src/icp_registration.cpp)
on the GPU (csrc/k_registration.hip) against a `ouster.sdk.core.VoxelHashMap3d`, and the adaptive threshold that goes with it
(adaptive_threshold.cpp).  Same names, keywords and defaults as the reference's binding; `build_linear_system` takes two (N, 3)
arrays (sources, targets) and returns (JtJ with the lower triangle filled, Jtr)."""
from ouster_sdk_amd.core import AdaptiveThreshold, ICPRegistration, build_linear_system  # noqa: F401
