"""mpcgpu_amd — MI355X-native PCG solver for MPCGPU's block-tridiagonal Schur system.

Product = libmpcg_hip.so (C ABI in include/mpcg.h and include/mpcg_riccati.h, kernels in mpcgpu_amd/csrc/).
This package is the thin host-side mirror of the reference's interface for that path.
"""
from .solver import Clocks, PcgSolver, Plant, QdldlSolver, XuRef, gain_blocks, pcg_config, pcgSharedMemSize  # noqa: F401

LdlSolver = QdldlSolver     # (the host LDL^T twin under its shorter name)

__all__ = ["Clocks", "PcgSolver", "Plant", "QdldlSolver", "XuRef", "LdlSolver", "gain_blocks", "pcg_config", "pcgSharedMemSize"]
