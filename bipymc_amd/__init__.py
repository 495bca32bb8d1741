"""bipymc_amd: MI355X-native DE-MC / DREAM population sampler.

Drop-in for the parallel samplers of wgurecky/bipymc (`bipymc.demc.DeMcMpi`,
`bipymc.dream.DreamMpi`): same constructor, `run_mcmc`, `param_est` and
`ln_like_fn` callback surface; the per-generation hot path runs as hand-written
HIP kernels behind the C ABI of include/bipymc_hip.h (libbipymc_hip.so).
"""
__version__ = "0.1.0"

from .demc import DeMcMpi  # noqa: F401
from .dream import DreamMpi  # noqa: F401
from .device_likelihood import HipLikelihood  # noqa: F401
from .covariance import PosteriorCovariance  # noqa: F401
from .histograms import PosteriorHistograms  # noqa: F401
from .traces import PosteriorTrace  # noqa: F401
from .derived import DerivedHistory, HipFunction, PosteriorDerived  # noqa: F401
from .pointwise import HipPointwise, PosteriorLoo, PosteriorWaic, compare_loo, compare_waic  # noqa: F401
from .summary import PosteriorHDI, PosteriorSummary  # noqa: F401
