"""A user-written likelihood at device speed: `ln_like_fn` given as HIP source.

The reference takes any Python callable as ln_like_fn (bipymc/samplers.py:36-43) and evaluates it row by row on the host; here that path is the
host callback (7-9e6 chain-updates/s at 8192 chains x 100 dimensions) or a device-resident framework callback (vectorized="device", 3e7).  A
likelihood written as a few lines of HIP C runs INSIDE the update kernel instead -- the library compiles its own update kernel around the function at
construction (hiprtc, about two seconds; include/bipymc_hip.h: bpm_set_device_likelihood), no host code per generation, 4e8 at that shape:

    ll = HipLikelihood('''
        __device__ double ln_like(const double* x, int d, const double* p) {      // p: the parameter block below (what ln_kwargs is to a callable)
            double s = 0.0;
            for (int j = 0; j < d; ++j) { const double z = (x[j] - p[j]) / p[d + j]; s += z * z; }
            return -0.5 * s;
        }''', params=np.concatenate([mu, sigma]))
    sampler = DreamMpi(ll, theta_0, n_chains=8192, ...)        # run_mcmc / param_est as ever

`python_fn` (optional): the same function for the host -- `ll(theta)` then works like any ln_like_fn (and the CPU test engine uses it)."""
import numpy as np


class HipLikelihood(object):
    """terms=K (optional, 1 ... 8): the PER-COORDINATE form for a likelihood that is a function of K sums over the coordinates.  `source` then defines

        __device__ void ln_like_terms(double xj, int j, int d, const double* p, double* acc)     // adds coordinate j's contribution into acc[0 .. K)
        __device__ double ln_like_finish(const double* acc, int d, const double* p)              // the value from the K sums

    instead of ln_like: inside the update kernel every lane of a chain adds the terms of its own coordinates and the sums meet in the kernel's reduction
    tree -- the shape of the shipped targets, and their speed (the plain form runs on one lane per chain).

    data=(n_data, w) float64 with terms=K (1 ... 8): the PER-DATUM form for a likelihood that is a function of K sums over the DATA -- a fit of a model
    with a few parameters to many data points, what every fitting script of the reference does.  `source` then defines

        __device__ void ln_like_datum(const double* x, int d, const double* y, int i, const double* p, double* acc)     // adds datum i (its w values: y) into acc[0 .. K)
        __device__ double ln_like_total(const double* x, int d, const double* acc, int n_data, const double* p)         // the value from the K sums; x: for a prior

    The data are copied to the device once; a wavefront per (proposal, chunk of the data) adds the terms, in an order that depends on n_data alone: the
    value of a point is a function of (x, data, params), bit for bit (csrc/user_eval_data.h).  A 1-D array is n_data values of w = 1.  Single rank."""

    MAX_DATA_W = 64

    def __init__(self, source, params=(), python_fn=None, terms=0, data=None):
        self.terms = int(terms)
        if not 0 <= self.terms <= 8:
            raise ValueError("terms must be 0 (plain ln_like) or 1 ... 8")
        self.data = None
        if data is not None:
            if self.terms < 1:
                raise ValueError("data needs terms=K (1 ... 8): the number of sums over the data")
            arr = np.asarray(data)
            if arr.dtype != np.float64:
                raise ValueError("data must be float64 (got %s)" % arr.dtype)
            if arr.ndim == 1:
                arr = arr.reshape(-1, 1)
            if arr.ndim != 2:
                raise ValueError("data must have shape (n_data, w) or (n_data,) (got %r)" % (arr.shape,))
            if not 1 <= arr.shape[0] < 2 ** 31:
                raise ValueError("data must have 1 <= n_data < 2^31 rows (got %d)" % arr.shape[0])
            if not 1 <= arr.shape[1] <= self.MAX_DATA_W:
                raise ValueError("data must have 1 <= w <= %d values per datum (got %d)" % (self.MAX_DATA_W, arr.shape[1]))
            self.data = np.ascontiguousarray(arr)
            self.source = "#define BPM_LN_LIKE_DATA %d\n#define BPM_LN_LIKE_DATA_W %d\n" % (self.terms, self.data.shape[1]) + str(source)
        else:
            self.source = ("#define BPM_LN_LIKE_TERMS %d\n" % self.terms if self.terms else "") + str(source)
        self.params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        self.python_fn = python_fn

    def __call__(self, theta, **kwargs):
        if self.python_fn is None:
            raise TypeError("this HipLikelihood has no python_fn: it can only be evaluated on the device")
        return self.python_fn(theta, **kwargs)

    def check(self, arch=None):
        """Compile only (no GPU needed): raises ValueError with the compiler's log when the source does not build for `arch` (default gfx950)."""
        from ._lib import check_source
        return check_source("bpm_check_device_likelihood", self.source.encode(), arch=arch)
