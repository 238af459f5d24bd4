"""`ouster.sdk.algorithm`: of the reference's algorithm package, the one function whose inputs this repo produces -- `normals`
(ouster_algorithm/src/normals.cpp), on the GPU (csrc/k_normals.hip).  Same call shapes and messages as the reference's binding."""
from ouster_sdk_amd.core import normals  # noqa: F401
