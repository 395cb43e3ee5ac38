/*
 * hhmm_stats_api.cpp -- the C ABI of the statistics per (series, draw) pair:
 * the E-step (include/hhmm_estep.h; its T-scan, hhmm_estep_scan.hip, too), the draw statistics (hhmm_gibbs.h,
 * hhmm_gibbs_gauss.h), the expected draw statistics (hhmm_expect.h), the IOHMM
 * E-step (hhmm_estep_io.h), the pointwise predictive densities
 * (hhmm_pointwise.h) and PSIS-LOO / -LFO on top of them (hhmm_psis.h).  They
 * share one host path: an entry is a row of StatsEntry (its check_* and launch_*
 * from hhmm_stats.h, its workspace, its arrays), and stats_check,
 * stats_workspace_size, stats_device and stats_host do the rest.  From
 * hhmm_api.cpp it takes the device pool, validate_impl, check_device and
 * hip_fail (hhmm_internal.h).
 */
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hhmm_internal.h"
#include "hhmm_stage.h"
#include "hhmm_stats.h"

using namespace hhmm;

/* One array of a host call: uploaded from host_in, or downloaded to host_out
 * after the launch; *dev is its pointer inside the device-side request /
 * result.  A row is live when its host pointer is non-NULL and it has bytes;
 * the device pointer of every other row is NULL. */
struct StatsArr {
    const void *host_in;
    void *host_out;
    void **dev;
    size_t bytes;
};

/* The device-side result of a host call, whichever struct the entry fills. */
union StatsResult {
    hhmm_estep_result estep;
    hhmm_estep_io_result io;
    hhmm_pointwise_result pw;
    hhmm_psis_result psis; /* psis.pw is pw */
};

/* What tells the entries apart on the host.  The result struct is the
 * entry's own: the shared path only hands it on. */
struct StatsEntry {
    const char *name; /* in messages */
    bool reads_u;     /* ffbs_u is an input (elsewhere the field is ignored) */
    hhmm_status (*check)(const hhmm_request *, const void *);
    hhmm_status (*launch)(const hhmm_request *, const void *, int64_t, void *, hipStream_t);
    size_t (*workspace)(const hhmm_request *req, int64_t P);
    /* the arrays of a host call: req / res on the host, dr / dq their device-side copies */
    void (*arrays)(const StatsEntry &en, const hhmm_request *req, const void *res, hhmm_request *dr, StatsResult *dq,
                   std::vector<StatsArr> &arrs);
    int k_lo = 1, k_hi = kMaxK;       /* the K its kernel takes (stats_check_k) */
    const char *below = "hhmm_estep"; /* the entry that takes K < k_lo */
    const char *above = nullptr;      /* where given: what a message says of K > k_hi */
};

/* The row of a state-parallel entry: its name, its uniforms and its K from its scope (hhmm_stats.h). */
static StatsEntry large_entry(const LkScope &sc, decltype(StatsEntry::check) check, decltype(StatsEntry::launch) launch,
                              decltype(StatsEntry::workspace) workspace, decltype(StatsEntry::arrays) arrays)
{
    return {sc.name, sc.reads_u, check, launch, workspace, arrays, sc.k_lo, sc.k_hi, sc.below};
}

template <class R, hhmm_status (*F)(const hhmm_request *, const R *)>
static hhmm_status typed_check(const hhmm_request *r, const void *o)
{
    return F(r, (const R *)o);
}
template <class R, hhmm_status (*F)(const hhmm_request *, const R *, int64_t, void *, hipStream_t)>
static hhmm_status typed_launch(const hhmm_request *r, const void *o, int64_t P, void *ws, hipStream_t st)
{
    return F(r, (const R *)o, P, ws, st);
}

/* hhmm_estep_result: the HMM and Tayal families */
static void estep_arrays(const StatsEntry &en, const hhmm_request *req, const void *res_, hhmm_request *dr_,
                         StatsResult *dq_, std::vector<StatsArr> &arrs)
{
    const hhmm_estep_result *res = (const hhmm_estep_result *)res_;
    hhmm_request &dr = *dr_;
    hhmm_estep_result &dq = dq_->estep;
    const hhmm_data &d = req->data;
    const hhmm_draws &w = req->draws;
    const size_t N = (size_t)d.n_series, S = (size_t)w.n_draws, Tm = (size_t)d.T_max, K = (size_t)d.K;
    const size_t P = (size_t)npairs(req);
    const bool gauss = req->model == HHMM_MODEL_HMM_GAUSS; /* else one of the discrete programs */
    const bool tayal = req->model == HHMM_MODEL_TAYAL;
    const bool semisup = req->model == HHMM_MODEL_HMM_MULTINOM_SEMISUP;
    const size_t L = gauss ? 0 : (size_t)d.L;
    arrs = {
        {d.T, nullptr, (void **)&dr.data.T, N * 4},
        {gauss ? nullptr : d.x_int, nullptr, (void **)&dr.data.x_int, N * Tm * 4},
        {gauss ? d.x_real : nullptr, nullptr, (void **)&dr.data.x_real, N * Tm * 8},
        {semisup ? d.g : nullptr, nullptr, (void **)&dr.data.g, N * Tm * 4},
        {tayal ? d.sign : nullptr, nullptr, (void **)&dr.data.sign, N * Tm * 4},
        {tayal ? nullptr : w.p_1k, nullptr, (void **)&dr.draws.p_1k, S * K * 8},
        {tayal ? nullptr : w.A_ij, nullptr, (void **)&dr.draws.A_ij, S * K * K * 8},
        {tayal ? w.p_11 : nullptr, nullptr, (void **)&dr.draws.p_11, S * 8},
        {tayal ? w.A_row : nullptr, nullptr, (void **)&dr.draws.A_row, S * 4 * 8},
        {gauss ? nullptr : w.phi_k, nullptr, (void **)&dr.draws.phi_k, S * K * L * 8},
        {gauss ? w.mu_k : nullptr, nullptr, (void **)&dr.draws.mu_k, S * K * 8},
        {gauss ? w.sigma_k : nullptr, nullptr, (void **)&dr.draws.sigma_k, S * K * 8},
        {en.reads_u ? req->ffbs_u : nullptr, nullptr, (void **)&dr.ffbs_u, P * Tm * 8},
        {nullptr, res->loglik, (void **)&dq.loglik, P * 8},
        {nullptr, res->n_1k, (void **)&dq.n_1k, P * K * 8},
        {nullptr, res->xi_ij, (void **)&dq.xi_ij, P * K * K * 8},
        {nullptr, gauss ? nullptr : res->c_kl, (void **)&dq.c_kl, P * K * L * 8},
        {nullptr, gauss ? res->w_k : nullptr, (void **)&dq.w_k, P * K * 8},
        {nullptr, gauss ? res->s1_k : nullptr, (void **)&dq.s1_k, P * K * 8},
        {nullptr, gauss ? res->s2_k : nullptr, (void **)&dq.s2_k, P * K * 8},
        {nullptr, res->pair_status, (void **)&dq.pair_status, P * 4},
    };
}

/* hhmm_estep_io_result: the IOHMM programs */
static void estep_io_arrays(const StatsEntry &, const hhmm_request *req, const void *res_, hhmm_request *dr_,
                            StatsResult *dq_, std::vector<StatsArr> &arrs)
{
    const hhmm_estep_io_result *res = (const hhmm_estep_io_result *)res_;
    hhmm_request &dr = *dr_;
    hhmm_estep_io_result &dq = dq_->io;
    const hhmm_data &d = req->data;
    const hhmm_draws &w = req->draws;
    const size_t N = (size_t)d.n_series, S = (size_t)w.n_draws, Tm = (size_t)d.T_max, K = (size_t)d.K;
    const size_t P = (size_t)npairs(req), M = (size_t)d.M;
    const bool reg = req->model == HHMM_MODEL_IOHMM_REG; /* else one of the mixture programs */
    const size_t L = reg ? 0 : (size_t)d.L;
    arrs = {
        {d.T, nullptr, (void **)&dr.data.T, N * 4},
        {d.x_real, nullptr, (void **)&dr.data.x_real, N * Tm * 8},
        {d.u, nullptr, (void **)&dr.data.u, N * Tm * M * 8},
        {w.p_1k, nullptr, (void **)&dr.draws.p_1k, S * K * 8},
        {w.w_km, nullptr, (void **)&dr.draws.w_km, S * K * M * 8},
        {reg ? w.b_km : nullptr, nullptr, (void **)&dr.draws.b_km, S * K * M * 8},
        {reg ? w.s_k : nullptr, nullptr, (void **)&dr.draws.s_k, S * K * 8},
        {reg ? nullptr : w.lambda_kl, nullptr, (void **)&dr.draws.lambda_kl, S * K * L * 8},
        {reg ? nullptr : w.mu_kl, nullptr, (void **)&dr.draws.mu_kl, S * K * L * 8},
        {reg ? nullptr : w.s_kl, nullptr, (void **)&dr.draws.s_kl, S * K * L * 8},
        {nullptr, res->loglik, (void **)&dq.loglik, P * 8},
        {nullptr, res->n_1k, (void **)&dq.n_1k, P * K * 8},
        {nullptr, res->gw_km, (void **)&dq.gw_km, P * K * M * 8},
        {nullptr, reg ? res->n_k : nullptr, (void **)&dq.n_k, P * K * 8},
        {nullptr, reg ? res->uu_kmm : nullptr, (void **)&dq.uu_kmm, P * K * M * M * 8},
        {nullptr, reg ? res->ux_km : nullptr, (void **)&dq.ux_km, P * K * M * 8},
        {nullptr, reg ? res->xx_k : nullptr, (void **)&dq.xx_k, P * K * 8},
        {nullptr, reg ? nullptr : res->n_kl, (void **)&dq.n_kl, P * K * L * 8},
        {nullptr, reg ? nullptr : res->sx_kl, (void **)&dq.sx_kl, P * K * L * 8},
        {nullptr, reg ? nullptr : res->sxx_kl, (void **)&dq.sxx_kl, P * K * L * 8},
        {nullptr, res->pair_status, (void **)&dq.pair_status, P * 4},
    };
}

/* hhmm_pointwise_result: the [N, T_max] reductions are N * T_max * 8 bytes; the
 * per-step arrays are uploaded too, so that a step t >= T[n] comes back as the
 * caller left it */
static void pointwise_arrays(const StatsEntry &, const hhmm_request *req, const void *res_, hhmm_request *dr_,
                             StatsResult *dq_, std::vector<StatsArr> &arrs)
{
    const hhmm_pointwise_result *res = (const hhmm_pointwise_result *)res_;
    hhmm_request &dr = *dr_;
    hhmm_pointwise_result &dq = dq_->pw;
    const hhmm_data &d = req->data;
    const hhmm_draws &w = req->draws;
    const size_t N = (size_t)d.n_series, S = (size_t)w.n_draws, Tm = (size_t)d.T_max, K = (size_t)d.K;
    const size_t P = (size_t)npairs(req);
    const bool gauss = req->model == HHMM_MODEL_HMM_GAUSS; /* else hmm-multinom */
    const size_t L = gauss ? 0 : (size_t)d.L;
    arrs = {
        {d.T, nullptr, (void **)&dr.data.T, N * 4},
        {gauss ? nullptr : d.x_int, nullptr, (void **)&dr.data.x_int, N * Tm * 4},
        {gauss ? d.x_real : nullptr, nullptr, (void **)&dr.data.x_real, N * Tm * 8},
        {w.p_1k, nullptr, (void **)&dr.draws.p_1k, S * K * 8},
        {w.A_ij, nullptr, (void **)&dr.draws.A_ij, S * K * K * 8},
        {gauss ? nullptr : w.phi_k, nullptr, (void **)&dr.draws.phi_k, S * K * L * 8},
        {gauss ? w.mu_k : nullptr, nullptr, (void **)&dr.draws.mu_k, S * K * 8},
        {gauss ? w.sigma_k : nullptr, nullptr, (void **)&dr.draws.sigma_k, S * K * 8},
        {nullptr, res->loglik, (void **)&dq.loglik, P * 8},
        {res->lpd_t, res->lpd_t, (void **)&dq.lpd_t, N * Tm * 8},
        {res->mean_t, res->mean_t, (void **)&dq.mean_t, N * Tm * 8},
        {res->var_t, res->var_t, (void **)&dq.var_t, N * Tm * 8},
        {res->lp_t, res->lp_t, (void **)&dq.lp_t, P * Tm * 8},
        {nullptr, res->pair_status, (void **)&dq.pair_status, P * 4},
    };
}

/* hhmm_psis_result: the pointwise arrays, then three more [N, T_max] arrays that make the round trip whole */
static void psis_arrays(const StatsEntry &en, const hhmm_request *req, const void *res_, hhmm_request *dr_,
                        StatsResult *dq_, std::vector<StatsArr> &arrs)
{
    const hhmm_psis_result *res = (const hhmm_psis_result *)res_;
    hhmm_psis_result &dq = dq_->psis;
    pointwise_arrays(en, req, &res->pw, dr_, dq_, arrs);
    const size_t cells = (size_t)req->data.n_series * (size_t)req->data.T_max * 8;
    arrs.push_back({res->elpd_t, res->elpd_t, (void **)&dq.elpd_t, cells});
    arrs.push_back({res->khat_t, res->khat_t, (void **)&dq.khat_t, cells});
    arrs.push_back({res->neff_t, res->neff_t, (void **)&dq.neff_t, cells});
}

static size_t no_workspace(const hhmm_request *, int64_t) { return 0; }
static size_t estep_workspace(const hhmm_request *req, int64_t P)
{
    return estep_workspace_bytes(req->data.K, req->data.T_max, P);
}

static const StatsEntry kEstep = {"E-step",
                                  false,
                                  typed_check<hhmm_estep_result, check_estep>,
                                  typed_launch<hhmm_estep_result, launch_estep>,
                                  estep_workspace,
                                  estep_arrays};
static const StatsEntry kEstepLarge =
    large_entry(kEstepLargeScope, typed_check<hhmm_estep_result, check_estep_large>,
                typed_launch<hhmm_estep_result, launch_estep_large>, lk_ckpt_workspace_bytes, estep_arrays);
static const StatsEntry kDrawStats = {"draw statistics",
                                      true,
                                      typed_check<hhmm_estep_result, check_draw_stats>,
                                      typed_launch<hhmm_estep_result, launch_draw_stats>,
                                      estep_workspace,
                                      estep_arrays};
static const StatsEntry kDrawStatsGauss = {"Gaussian draw statistics",
                                           true,
                                           typed_check<hhmm_estep_result, check_draw_stats_gauss>,
                                           typed_launch<hhmm_estep_result, launch_draw_stats_gauss>,
                                           estep_workspace,
                                           estep_arrays};
static const StatsEntry kDrawStatsLarge =
    large_entry(kDrawStatsLargeScope, typed_check<hhmm_estep_result, check_draw_stats_large>,
                typed_launch<hhmm_estep_result, launch_draw_stats_large>, lk_ckpt_workspace_bytes, estep_arrays);
static const StatsEntry kExpectedStats = {"expected statistics",
                                          false,
                                          typed_check<hhmm_estep_result, check_expected_stats>,
                                          typed_launch<hhmm_estep_result, launch_expected_stats>,
                                          estep_workspace,
                                          estep_arrays};
/* the T-scan of both (hhmm_estep_scan.hip): one launch and one workspace, the checks of their twins */
static const StatsEntry kEstepScan = {"T-scan E-step",
                                      false,
                                      typed_check<hhmm_estep_result, check_estep_scan>,
                                      typed_launch<hhmm_estep_result, launch_estep_scan>,
                                      estep_scan_workspace_bytes,
                                      estep_arrays,
                                      1,
                                      kMaxK,
                                      "hhmm_estep",
                                      kEstepScanAbove};
static const StatsEntry kExpectedStatsScan = {"T-scan expected statistics",
                                              false,
                                              typed_check<hhmm_estep_result, check_expected_stats_scan>,
                                              typed_launch<hhmm_estep_result, launch_estep_scan>,
                                              estep_scan_workspace_bytes,
                                              estep_arrays,
                                              1,
                                              kMaxK,
                                              "hhmm_estep",
                                              kEstepScanAbove};
static const StatsEntry kPointwise = {"pointwise",
                                      false,
                                      typed_check<hhmm_pointwise_result, check_pointwise>,
                                      typed_launch<hhmm_pointwise_result, launch_pointwise>,
                                      pointwise_workspace_bytes,
                                      pointwise_arrays};
static const StatsEntry kPointwiseLarge =
    large_entry(kPointwiseLargeScope, typed_check<hhmm_pointwise_result, check_pointwise_large>,
                typed_launch<hhmm_pointwise_result, launch_pointwise_large>, pointwise_large_workspace_bytes,
                pointwise_arrays);
static const StatsEntry kPsisLoo = {"PSIS-LOO",
                                    false,
                                    typed_check<hhmm_psis_result, check_psis>,
                                    typed_launch<hhmm_psis_result, launch_psis_loo>,
                                    psis_loo_workspace_bytes,
                                    psis_arrays,
                                    1,
                                    kMaxKLarge};
static const StatsEntry kPsisLfo = {"PSIS-LFO",
                                    false,
                                    typed_check<hhmm_psis_result, check_psis>,
                                    typed_launch<hhmm_psis_result, launch_psis_lfo>,
                                    psis_lfo_workspace_bytes,
                                    psis_arrays,
                                    1,
                                    kMaxKLarge};
static const StatsEntry kEstepIo = {"IOHMM E-step",
                                    false,
                                    typed_check<hhmm_estep_io_result, check_estep_io>,
                                    typed_launch<hhmm_estep_io_result, launch_estep_io>,
                                    no_workspace,
                                    estep_io_arrays};

/* Argument checks of the device and the host entry, none of which needs a
 * device: the entry's own scope first (HHMM_ERR_UNSUPPORTED names the reason),
 * then the request as hhmm_run / hhmm_run_device check it (host: the
 * data-block bounds too). */
static hhmm_status stats_check(const StatsEntry &en, const hhmm_request *req, const void *res, bool host)
{
    hhmm_status s = en.check(req, res);
    if (s != HHMM_OK)
        return s;
    hhmm_request r2 = *req; /* outputs and hat_rand are ignored, ffbs_u unless the entry reads it */
    r2.outputs = HHMM_OUT_LOGLIK;
    r2.hat_rand = nullptr;
    if (!en.reads_u)
        r2.ffbs_u = nullptr;
    return validate_impl(&r2, nullptr, host);
}

static hhmm_status stats_workspace_size(const StatsEntry &en, const hhmm_request *req, size_t *bytes)
{
    if (!req || !bytes) {
        set_error("NULL argument");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const int64_t P = npairs(req);
    if (P < 1 || req->data.K < 1 || req->data.T_max < 1) {
        set_error("request describes no pairs");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (stats_check_k(en.name, req->data.K, en.k_lo, en.k_hi, en.below, en.above) != HHMM_OK)
        return HHMM_ERR_UNSUPPORTED;
    *bytes = en.workspace(req, P);
    return HHMM_OK;
}

static hhmm_status stats_device(const StatsEntry &en, const hhmm_request *req, const void *res, void *workspace,
                                size_t workspace_bytes_, void *stream)
{
    hhmm_status s = stats_check(en, req, res, false);
    if (s != HHMM_OK)
        return s;
    if ((s = check_device()) != HHMM_OK)
        return s;
    const int64_t P = npairs(req);
    const size_t need = en.workspace(req, P);
    if (workspace_bytes_ < need || (need && !workspace)) {
        set_error("workspace of %zu bytes < %zu required", workspace_bytes_, need);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return en.launch(req, res, P, workspace, (hipStream_t)stream);
}

static hhmm_status stats_host(const StatsEntry &en, const hhmm_request *req, const void *res)
{
    hhmm_status s = stats_check(en, req, res, true);
    if (s != HHMM_OK)
        return s;
    if ((s = check_device()) != HHMM_OK)
        return s;
    int dev = req->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess)
        return hip_fail(hipGetLastError(), "hipGetDevice");
    hipError_t e = hipSetDevice(dev);
    if (e != hipSuccess)
        return hip_fail(e, "hipSetDevice");
    const size_t P = (size_t)npairs(req);
    hhmm_request dr = *req;
    StatsResult dq{};
    std::vector<StatsArr> arrs;
    en.arrays(en, req, res, &dr, &dq, arrs);
    /* one pooled block: every array at a 256-byte boundary, then the workspace */
    size_t total = 0;
    std::vector<size_t> off;
    for (const StatsArr &a : arrs) {
        off.push_back(total);
        if ((a.host_in || a.host_out) && a.bytes)
            total += (a.bytes + 255) & ~(size_t)255;
    }
    const size_t wsb = en.workspace(req, (int64_t)P);
    char *blk = (char *)pool_get(dev, total);
    void *ws = pool_get(dev, wsb);
    auto cleanup = [&]() {
        pool_put(blk);
        pool_put(ws);
    };
    if (!blk || !ws) {
        cleanup();
        set_error("device %d: %s allocation of %zu + %zu bytes failed", dev, en.name, total, wsb);
        return HHMM_ERR_OUT_OF_MEMORY;
    }
    for (size_t i = 0; i < arrs.size() && e == hipSuccess; ++i) {
        const StatsArr &a = arrs[i];
        const bool used = (a.host_in || a.host_out) && a.bytes;
        *a.dev = used ? (void *)(blk + off[i]) : nullptr;
        if (used && a.host_in)
            e = hipMemcpy(*a.dev, a.host_in, a.bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        cleanup();
        return hip_fail(e, (std::string(en.name) + " upload").c_str());
    }
    s = en.launch(&dr, &dq, (int64_t)P, ws, nullptr);
    e = hipStreamSynchronize(nullptr); /* before the pooled blocks can go to another request */
    if (s == HHMM_OK && e == hipSuccess)
        for (const StatsArr &a : arrs)
            if (a.host_out && a.bytes && e == hipSuccess)
                e = hipMemcpy(a.host_out, *a.dev, a.bytes, hipMemcpyDeviceToHost);
    cleanup();
    if (s != HHMM_OK)
        return s;
    if (e != hipSuccess)
        return hip_fail(e, (std::string(en.name) + " (kernel execution or download)").c_str());
    return HHMM_OK;
}

extern "C" {

hhmm_status hhmm_estep_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kEstep, req, bytes);
}
hhmm_status hhmm_estep_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace, size_t workspace_bytes_,
                              void *stream)
{
    return stats_device(kEstep, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_estep(const hhmm_request *req, hhmm_estep_result *res) { return stats_host(kEstep, req, res); }

hhmm_status hhmm_estep_large_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kEstepLarge, req, bytes);
}
hhmm_status hhmm_estep_large_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                    size_t workspace_bytes_, void *stream)
{
    return stats_device(kEstepLarge, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_estep_large(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kEstepLarge, req, res);
}

hhmm_status hhmm_estep_scan_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kEstepScan, req, bytes);
}
hhmm_status hhmm_estep_scan_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                   size_t workspace_bytes_, void *stream)
{
    return stats_device(kEstepScan, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_estep_scan(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kEstepScan, req, res);
}
hhmm_status hhmm_estep_scan_plan(const hhmm_request *req, int32_t *chunk_len, int32_t *n_chunks)
{
    if (!req || !chunk_len || !n_chunks || npairs(req) < 1) {
        set_error("NULL argument, or a request that describes no pairs");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const ScanPlan sp = estep_scan_plan(req->model, req->data.K, req->data.L, req->data.T_max, npairs(req),
                                        (uint32_t)req->flags);
    *chunk_len = sp.cl;
    *n_chunks = sp.nc;
    return HHMM_OK;
}

hhmm_status hhmm_expected_stats_scan_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kExpectedStatsScan, req, bytes);
}
hhmm_status hhmm_expected_stats_scan_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                            size_t workspace_bytes_, void *stream)
{
    return stats_device(kExpectedStatsScan, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_expected_stats_scan(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kExpectedStatsScan, req, res);
}

hhmm_status hhmm_draw_stats_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kDrawStats, req, bytes);
}
hhmm_status hhmm_draw_stats_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                   size_t workspace_bytes_, void *stream)
{
    return stats_device(kDrawStats, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_draw_stats(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kDrawStats, req, res);
}

hhmm_status hhmm_draw_stats_gauss_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kDrawStatsGauss, req, bytes);
}
hhmm_status hhmm_draw_stats_gauss_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                         size_t workspace_bytes_, void *stream)
{
    return stats_device(kDrawStatsGauss, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_draw_stats_gauss(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kDrawStatsGauss, req, res);
}

hhmm_status hhmm_draw_stats_large_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kDrawStatsLarge, req, bytes);
}
hhmm_status hhmm_draw_stats_large_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                         size_t workspace_bytes_, void *stream)
{
    return stats_device(kDrawStatsLarge, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_draw_stats_large(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kDrawStatsLarge, req, res);
}

hhmm_status hhmm_expected_stats_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kExpectedStats, req, bytes);
}
hhmm_status hhmm_expected_stats_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                       size_t workspace_bytes_, void *stream)
{
    return stats_device(kExpectedStats, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_expected_stats(const hhmm_request *req, hhmm_estep_result *res)
{
    return stats_host(kExpectedStats, req, res);
}

hhmm_status hhmm_estep_io_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kEstepIo, req, bytes);
}
hhmm_status hhmm_estep_io_device(const hhmm_request *req, hhmm_estep_io_result *res, void *workspace,
                                 size_t workspace_bytes_, void *stream)
{
    return stats_device(kEstepIo, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_estep_io(const hhmm_request *req, hhmm_estep_io_result *res)
{
    return stats_host(kEstepIo, req, res);
}

hhmm_status hhmm_pointwise_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kPointwise, req, bytes);
}
hhmm_status hhmm_pointwise_device(const hhmm_request *req, hhmm_pointwise_result *res, void *workspace,
                                  size_t workspace_bytes_, void *stream)
{
    return stats_device(kPointwise, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_pointwise(const hhmm_request *req, hhmm_pointwise_result *res)
{
    return stats_host(kPointwise, req, res);
}

hhmm_status hhmm_pointwise_large_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kPointwiseLarge, req, bytes);
}
hhmm_status hhmm_pointwise_large_device(const hhmm_request *req, hhmm_pointwise_result *res, void *workspace,
                                        size_t workspace_bytes_, void *stream)
{
    return stats_device(kPointwiseLarge, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_pointwise_large(const hhmm_request *req, hhmm_pointwise_result *res)
{
    return stats_host(kPointwiseLarge, req, res);
}

hhmm_status hhmm_psis_loo_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kPsisLoo, req, bytes);
}
hhmm_status hhmm_psis_loo_device(const hhmm_request *req, hhmm_psis_result *res, void *workspace,
                                 size_t workspace_bytes_, void *stream)
{
    return stats_device(kPsisLoo, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_psis_loo(const hhmm_request *req, hhmm_psis_result *res) { return stats_host(kPsisLoo, req, res); }

hhmm_status hhmm_psis_lfo_workspace_size(const hhmm_request *req, size_t *bytes)
{
    return stats_workspace_size(kPsisLfo, req, bytes);
}
hhmm_status hhmm_psis_lfo_device(const hhmm_request *req, hhmm_psis_result *res, void *workspace,
                                 size_t workspace_bytes_, void *stream)
{
    return stats_device(kPsisLfo, req, res, workspace, workspace_bytes_, stream);
}
hhmm_status hhmm_psis_lfo(const hhmm_request *req, hhmm_psis_result *res) { return stats_host(kPsisLfo, req, res); }

} // extern "C"
