"""ginkgo_amd - MI355X (gfx950 / CDNA4) backend for Ginkgo's Krylov hot path.

Thin host-side mirror of the gko::Executor / gko::LinOp / solver-factory
interface over the C ABI of libgko_cdna4.so (include/gko_cdna4.h): CSR / ELL /
SELL-P / Fbcsr SpMV, block-Jacobi, level-scheduled triangular solves with Sor / SSOR, ILU(0) / IC(0) with Ilu / Ic (exact, by the fixed-point sweeps of factorization.ParIlu / ParIc, or with threshold fill-in by factorization.ParIlut / ParIct), triangular ISAI (LowerIsai / UpperIsai), general and spd ISAI (GeneralIsai / SpdIsai), Pgm aggregation and a Multigrid solver / preconditioner, sparse direct factorizations with a nested-dissection reordering (reorder.NestedDissection, Permutation, reorder.ScaledReordered), batched Cg / Bicgstab on batch Csr / Ell (ginkgo_amd.batch), BLAS-1 and the fused CG steps as hand-written HIP
kernels.  Importing the package does not need a GPU; creating a
Cdna4Executor does, and there is no CPU fallback.
"""
from ._lib import (DimensionMismatch, GkoError, NotCompiled, NotSupported,
                   LIB_PATH)
from .executor import Cdna4Executor
from .matrix import (Coo, Csr, Dense, DeviceMatrixData, Ell, Fbcsr, Hybrid, Permutation, Sellp, entry_dtype, scalar,
                     stencil_csr)
from .preconditioner import GaussSeidel, Ic, Ilu, Jacobi, Sor, compute_storage_scheme
from .triangular import Direct, LowerTrs, UpperTrs
from .isai import GeneralIsai, LowerIsai, SpdIsai, UpperIsai
from .multigrid import Multigrid, Pgm
from . import multigrid
from . import batch
from . import factorization
from . import reorder
from .reorder import NestedDissection, ScaledReordered
from .solver import Cg, Gmres, Identity, ortho_method
from .krylov import Bicg, Bicgstab, Cgs, Chebyshev, Fcg, Gcr, Ir, Minres, PipeCg
from . import stop

__all__ = ["LowerTrs", "UpperTrs", "Direct", "LowerIsai", "UpperIsai", "GeneralIsai", "SpdIsai", "Pgm", "Multigrid", "multigrid", "batch", "Sor", "GaussSeidel", "Ilu", "Ic", "factorization", "reorder", "NestedDissection", "ScaledReordered", "Permutation", "Coo", "DeviceMatrixData", "entry_dtype", "Hybrid", "Bicg", "Bicgstab", "Chebyshev", "Gcr", "Ir", "Minres", "Cgs", "Fcg", "PipeCg", "Cdna4Executor", "Csr", "Dense", "Ell", "Fbcsr", "Sellp", "scalar",
           "stencil_csr", "Jacobi", "compute_storage_scheme", "Cg", "Gmres", "ortho_method", "Identity",
           "stop", "GkoError", "NotCompiled", "NotSupported",
           "DimensionMismatch", "LIB_PATH"]
