"""`ouster.sdk.algorithm`: of the reference's algorithm package, the functions whose inputs this repo produces -- `normals`
(ouster_algorithm/src/normals.cpp) on the GPU (csrc/k_normals.hip), and `point_to_point_align` / `point_to_plane_align`
(ouster_algorithm/src/align_clouds.cpp) on the GPU (csrc/k_icp.hip).  Same call shapes and messages as the reference's binding.
`IcpTarget` is a project extension the reference does not have: a target kept on the GPU and many sources aligned per call."""
from ouster_sdk_amd.core import IcpTarget, normals, point_to_plane_align, point_to_point_align  # noqa: F401
