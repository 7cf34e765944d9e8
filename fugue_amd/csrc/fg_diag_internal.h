// fg_diag_internal.h -- what fg_diag.hip shares with fg_diag_stream.hip: the context of the two combination callbacks and the
// combination itself once the per-chain moments are on the device.  Both producers of moments and lag sums (a stored draw buffer,
// a stream of chunks) go through the same reduce / all-reduce / gather code.
#pragma once
#include "fg_engine_internal.h"

struct fg_diag_stream;

// `sums` (NULL: k_diag_autocov over d_draws) leaves this engine's pooled lag sums d_sums [d][n_lags] on the device, synchronised.
struct AcovCtx {
    fg_engine *e; const double *d_draws; int n, d; const double *d_mom; void *comm; double *d_small; double *d_part; long long bytes;
    int (*sums)(AcovCtx *A, int lag0, int n_lags, double *d_sums) = nullptr;
    fg_diag_stream *src = nullptr;
};

// k_diag_acov_finish over block partials [d][32][nblk] -> d_sums [d][n_lags], then a synchronise of the engine's stream
int fg_diag_finish_lag_sums(fg_engine *e, const double *d_part, int nblk, int n_lags, int d, double *d_sums);

// fg_diag_rhat_ess after its moments kernel: d_mom [d][6][C], d_res [d][C] (needed when h_std is asked for) on the device; `proto`
// carries d_draws or (sums, src).  Owns nothing it is handed.
int fg_diag_rhat_ess_from_moments(fg_engine *e, int n, int d, void *comm, const double *d_mom, const double *d_res, const AcovCtx &proto,
                                  double *h_rhat, double *h_ess, double *h_mean, double *h_std, int64_t *out_total_chains);
