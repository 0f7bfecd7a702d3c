"""gprc on MI355X: the GP predict hot path of the R package `gprc`
(MoHawastaken/Gaussian-Process-Regression) behind the reference's own API surface.

Host mirror of the R6 / cov_func interface (reference R/GPRclass.R, R/GPCclass.R) over the C ABI of
include/gprc_native.h; all matrix arithmetic runs in hand-written HIP kernels for gfx950.  There is no
CPU fallback: without the built library / an MI355X the compute calls raise.
"""
from . import _native
from ._native import GprcError, NotPositiveDefinite, Context, default_context, device_count
from .covfunc import (cov_func, covariance_matrix, constant, linear, polynomial, sqrexp, gammaexp,
                      rationalquadratic, sqrexp_ard, matern32, matern52, matern32_ard, matern52_ard, CovFunc)
from .gpr import (GPR, GPR_constant, GPR_linear, GPR_polynomial, GPR_sqrexp, GPR_gammaexp,
                  GPR_rationalquadratic, GPR_sqrexp_ard, GPR_matern32, GPR_matern52, GPR_matern32_ard, GPR_matern52_ard)
from .gpc import GPC
from .fit import fit, dens, dens_deriv, logp_grad, logp_grad_batch, optimize, optimize_multistart, logq_grad, optimize_gpc, elbo_grad, optimize_sparse, iter_logp_grad, optimize_iterative, vecchia_logp_grad, optimize_local
from .batch import BatchGPR, BatchGPC
from .sparse import SparseGPR, select_inducing
from .iterative import IterativeGPR, EvidenceEstimate
from .local import LocalGPR, LocalGPC, knn, knn_before, vecchia_order
from .sampling import multivariate_normal, expand_range, mvn_factor, sym_eigen, spectral_frequencies, SamplePaths, PathMaxima, maximize_paths
from .simulation import combine_all, iid_noise, simulate_regression, simulate_regression_gp, simulate_classification

__all__ = ["LocalGPR", "LocalGPC", "BatchGPC", "knn", "knn_before", "vecchia_order", "vecchia_logp_grad", "optimize_local", "BatchGPR", "logp_grad_batch", "optimize_multistart", "SparseGPR", "IterativeGPR", "EvidenceEstimate", "iter_logp_grad", "optimize_iterative", "select_inducing", "elbo_grad", "optimize_sparse", "fit", "dens", "dens_deriv", "logp_grad", "optimize", "logq_grad", "optimize_gpc", "sqrexp_ard", "GPR_sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard",
           "GPR_matern32", "GPR_matern52", "GPR_matern32_ard", "GPR_matern52_ard", "multivariate_normal", "expand_range", "mvn_factor", "sym_eigen", "spectral_frequencies", "SamplePaths", "PathMaxima", "maximize_paths", "combine_all", "iid_noise",
           "simulate_regression", "simulate_regression_gp", "simulate_classification", "GPR", "GPR_constant", "GPR_linear", "GPR_polynomial", "GPR_sqrexp", "GPR_gammaexp",
           "GPR_rationalquadratic", "GPC", "cov_func", "covariance_matrix", "constant", "linear", "polynomial",
           "sqrexp", "gammaexp", "rationalquadratic", "CovFunc", "GprcError", "NotPositiveDefinite", "Context",
           "default_context", "device_count"]
