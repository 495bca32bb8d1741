// DEVICE CODE OF A RUN-TIME PROGRAM (hiprtc; user_likelihood.h hands it over as an embedded header): ln_like for a caller's source in the
// per-coordinate form, derived from its ln_like_terms / ln_like_finish.  Included behind the caller's source by every program built around a
// likelihood (user_eval.h, user_target.h); a source in the plain form defines ln_like itself and gets nothing from here.

#ifdef BPM_LN_LIKE_TERMS
__device__ double ln_like(const double* x, int d, const double* p) {
    double acc[BPM_LN_LIKE_TERMS];
    for (int k = 0; k < BPM_LN_LIKE_TERMS; ++k) acc[k] = 0.0;
    for (int j = 0; j < d; ++j) ln_like_terms(x[j], j, d, p, acc);
    return ln_like_finish(acc, d, p);
}
#endif
