/*
 * hhmm_api.cpp -- the C ABI of libhhmm.so (include/hhmm.h).
 *
 * Host side of the drop-in boundary: validates a request the way Stan's data
 * block and parameter constraints would (declared bounds such as
 * `int<lower=1, upper=L> x[T]`, hmm/stan/hmm-multinom.stan:12), sizes the
 * workspace, moves host arrays to and from the device for the R path
 * (hhmm_run; its plan and host staging are hhmm_stage.cpp), and launches the
 * gfx950 kernels (hhmm_kernels.hip).  There is no CPU compute path: without a
 * gfx950 device every entry point fails with HHMM_ERR_NO_DEVICE.
 */
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <algorithm>

#include "hhmm_internal.h"
#include "hhmm_stage.h"
#include "build_id.h" /* HHMM_SOURCE_HASH (Makefile) */

namespace hhmm {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

/* ---------------- device pool (per device, size-bucketed) ---------------- */
struct Pool {
    std::mutex mu;
    std::map<int, std::multimap<size_t, void *>> free_blocks;
    std::map<void *, std::pair<int, size_t>> live;
};
static Pool &pool()
{
    static Pool p;
    return p;
}

void *pool_get(int dev, size_t bytes)
{
    if (bytes == 0)
        bytes = 256;
    bytes = (bytes + 4095) & ~(size_t)4095;
    Pool &p = pool();
    {
        std::lock_guard<std::mutex> g(p.mu);
        auto &fb = p.free_blocks[dev];
        auto it = fb.lower_bound(bytes);
        if (it != fb.end() && it->first <= bytes + bytes / 4) {
            void *ptr = it->second;
            p.live[ptr] = {dev, it->first};
            fb.erase(it);
            return ptr;
        }
    }
    void *ptr = nullptr;
    if (hipMalloc(&ptr, bytes) != hipSuccess) {
        /* release cached blocks of this device and retry once */
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> g(p.mu);
            for (auto &kv : p.free_blocks[dev])
                drop.push_back(kv.second);
            p.free_blocks[dev].clear();
        }
        for (void *q : drop)
            (void)hipFree(q);
        (void)hipGetLastError();
        if (hipMalloc(&ptr, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    std::lock_guard<std::mutex> g(p.mu);
    p.live[ptr] = {dev, bytes};
    return ptr;
}

void pool_put(void *ptr)
{
    if (!ptr)
        return;
    Pool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    auto it = p.live.find(ptr);
    if (it == p.live.end())
        return;
    p.free_blocks[it->second.first].emplace(it->second.second, ptr);
    p.live.erase(it);
}

/* ---------------- side streams (one per device) ---------------- */
struct SideStreams {
    std::mutex mu;
    std::map<int, std::pair<hipStream_t, hipEvent_t>> by_dev; /* key dev * 2 + high priority: stream, fork event */
    std::map<int, hipEvent_t> join_ev;
};
static SideStreams &side_streams()
{
    static SideStreams s;
    return s;
}

hhmm_status fork_stream(hipStream_t st, hipStream_t *side)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_error("hipGetDevice failed");
        return HHMM_ERR_HIP;
    }
    SideStreams &ss = side_streams();
    /* The side pass (the decoder beside the forward-backward) runs on a
     * high-priority stream: at C5 its chain of V-scan kernels is the critical
     * path, and the forward-backward scan's waves fill in around it (13.37 ->
     * 12.71 ms interleaved on one box, profiles/r03s_ab_c5_side_prio.log).
     * Probe knob HHMM_PROBE_SIDE_PRIO=0: a normal-priority side stream. */
    const char *pk = probe_env("HHMM_PROBE_SIDE_PRIO");
    const int hi = (pk && pk[0] == '0') ? 0 : 1;
    const int key = dev * 2 + hi;
    std::lock_guard<std::mutex> g(ss.mu);
    auto it = ss.by_dev.find(key);
    if (it == ss.by_dev.end()) {
        hipStream_t s2 = nullptr;
        hipEvent_t ev = nullptr, ej = nullptr;
        int lo_p = 0, hi_p = 0;
        if (hi)
            (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
        if (hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, hi ? hi_p : 0) != hipSuccess ||
            hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ej, hipEventDisableTiming) != hipSuccess) {
            set_error("side stream creation failed");
            return HHMM_ERR_HIP;
        }
        it = ss.by_dev.emplace(key, std::make_pair(s2, ev)).first;
        ss.join_ev[key] = ej;
    }
    if (hipEventRecord(it->second.second, st) != hipSuccess ||
        hipStreamWaitEvent(it->second.first, it->second.second, 0) != hipSuccess) {
        set_error("stream fork failed");
        return HHMM_ERR_HIP;
    }
    *side = it->second.first;
    return HHMM_OK;
}

hhmm_status join_stream(hipStream_t st, hipStream_t side)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_error("hipGetDevice failed");
        return HHMM_ERR_HIP;
    }
    SideStreams &ss = side_streams();
    std::lock_guard<std::mutex> g(ss.mu);
    hipEvent_t ej = nullptr;
    for (int hi = 0; hi < 2 && !ej; ++hi) /* the side stream is the one `side` names */
        if (ss.by_dev.count(dev * 2 + hi) && ss.by_dev[dev * 2 + hi].first == side)
            ej = ss.join_ev[dev * 2 + hi];
    if (!ej || hipEventRecord(ej, side) != hipSuccess || hipStreamWaitEvent(st, ej, 0) != hipSuccess) {
        set_error("stream join failed");
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

/* Waits for a request's work: its own stream and, when this device has one,
 * the library's side stream (a failed launch can leave a forked kernel there
 * unjoined).  Other streams -- other threads' requests -- are not waited on. */
static hipError_t sync_request(hipStream_t st)
{
    hipError_t e = hipStreamSynchronize(st);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return e;
    SideStreams &ss = side_streams();
    for (int hi = 0; hi < 2; ++hi) {
        hipStream_t side = nullptr;
        {
            std::lock_guard<std::mutex> g(ss.mu);
            auto it = ss.by_dev.find(dev * 2 + hi);
            if (it != ss.by_dev.end())
                side = it->second.first;
        }
        if (side) {
            hipError_t e2 = hipStreamSynchronize(side);
            if (e == hipSuccess)
                e = e2;
        }
    }
    return e;
}

static void pool_release_all()
{
    Pool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    for (auto &dv : p.free_blocks) {
        (void)hipSetDevice(dv.first);
        for (auto &kv : dv.second)
            (void)hipFree(kv.second);
    }
    p.free_blocks.clear();
}

/* ---------------- request description ---------------- */

/* Outputs each Stan program declares (TP / GQ names); the
 * output classes and model predicates are hhmm_plan.h's. */
static uint32_t available_outputs(int m)
{
    const uint32_t fb = kOutFb | kOutVit;
    /* FFBS (the engine's contract, §8 A14) is offered wherever the program has
     * a forward filter over the full series and a backward pass */
    if (hmm_has_backward(m))
        return fb | HHMM_OUT_FFBS;
    switch (m) {
    case HHMM_MODEL_IOHMM_REG:
    case HHMM_MODEL_IOHMM_MIX:
        /* + the fitted-output GQ draws (iohmm-reg.stan:124-148; iohmm-mix.stan:133-161) */
        return fb | HHMM_OUT_OBLIK_TK | HHMM_OUT_LOGA | HHMM_OUT_FFBS | HHMM_OUT_HATPI | HHMM_OUT_HATZ |
               HHMM_OUT_HATX | (m == HHMM_MODEL_IOHMM_MIX ? HHMM_OUT_HATL : 0u);
    case HHMM_MODEL_IOHMM_HMIX: /* hatpi_tk is a local there (iohmm-hmix.stan:147) */
        return HHMM_OUT_LOGLIK | HHMM_OUT_UNALPHA | HHMM_OUT_ALPHA | HHMM_OUT_BETA | HHMM_OUT_GAMMA |
               HHMM_OUT_OBLIK_TK | HHMM_OUT_OBLIK_T | HHMM_OUT_LOGA | HHMM_OUT_ZSTAR | HHMM_OUT_LOGP_ZSTAR |
               HHMM_OUT_FFBS | HHMM_OUT_HATZ | HHMM_OUT_HATL | HHMM_OUT_HATX;
    case HHMM_MODEL_IOHMM_HMIX_LITE:
        return HHMM_OUT_LOGLIK | HHMM_OUT_UNALPHA | HHMM_OUT_OBLIK_TK | HHMM_OUT_OBLIK_T | HHMM_OUT_LOGA;
    case HHMM_MODEL_TAYAL_LITE:
        return HHMM_OUT_LOGLIK | HHMM_OUT_UNALPHA | HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA_OOS | HHMM_OUT_ALPHA_OOS |
               HHMM_OUT_ZSTAR | HHMM_OUT_LOGP_ZSTAR;
    default:
        return 0;
    }
}

/* Models with a gfx950 path in this build. */
static bool device_supported(int m)
{
    return m >= HHMM_MODEL_HMM_GAUSS && m <= HHMM_MODEL_TAYAL_LITE;
}

#define REQUIRE(cond, ...)                                                                          \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            set_error(__VA_ARGS__);                                                                 \
            return HHMM_ERR_INVALID_ARGUMENT;                                                       \
        }                                                                                           \
    } while (0)

/* 1 when some element v[n + N t] with t < T[n] (T null: every t < Tm) lies
 * outside [lo, hi].  Time-major, so each thread streams contiguous rows (the
 * n-major loop that names the first offender in the error message strides by
 * N and took ~0.2 s at C2-host's 2e8 symbols); threads over time ranges for
 * large arrays.  The distance from lo is taken in unsigned arithmetic: R's
 * NA_integer_ is INT32_MIN, and INT32_MIN - lo overflows a signed int. */
static bool any_out_of_range(const int32_t *v, int64_t N, int Tm, const int32_t *T, int32_t lo, int32_t hi)
{
    const uint32_t span = (uint32_t)(hi - lo);
    auto rows = [&](int t0, int t1) {
        bool bad = false;
        for (int t = t0; t < t1 && !bad; ++t) {
            const int32_t *r = v + N * (int64_t)t;
            if (!T) {
                uint32_t acc = 0;
                for (int64_t n = 0; n < N; ++n)
                    acc |= (uint32_t)((uint32_t)r[n] - (uint32_t)lo > span);
                bad = acc != 0;
            } else {
                for (int64_t n = 0; n < N; ++n)
                    bad |= (t < T[n]) & ((uint32_t)r[n] - (uint32_t)lo > span);
            }
        }
        return bad;
    };
    const int64_t total = N * (int64_t)Tm;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nt = total < (int64_t(1) << 22) ? 1 : (int)std::min<int64_t>(std::min(16u, hw), Tm);
    if (nt <= 1)
        return rows(0, Tm);
    std::vector<char> res((size_t)nt, 0);
    run_parallel((size_t)nt, [&](size_t i) {
        res[i] = rows((int)((int64_t)Tm * (int64_t)i / nt), (int)((int64_t)Tm * (int64_t)(i + 1) / nt));
    });
    for (char c : res)
        if (c)
            return true;
    return false;
}

/* o == nullptr: the request side only (the segment summary call has no result). */
hhmm_status validate_impl(const hhmm_request *r, const hhmm_result *o, bool host)
{
    REQUIRE(r, "request must be non-NULL");
    REQUIRE(r->abi_version == HHMM_ABI_VERSION, "abi_version %u != %u", r->abi_version, HHMM_ABI_VERSION);
    REQUIRE(r->model >= 1 && r->model <= 9, "unknown model id %d", r->model);
    REQUIRE(r->pairing == HHMM_PAIR_GRID || r->pairing == HHMM_PAIR_ZIP || r->pairing == HHMM_PAIR_BLOCK,
            "unknown pairing %d", r->pairing);
    const hhmm_data &d = r->data;
    const hhmm_draws &w = r->draws;
    REQUIRE(d.n_series >= 1, "n_series must be >= 1");
    REQUIRE(w.n_draws >= 1, "n_draws must be >= 1");
    REQUIRE(npairs(r) >= 1, "%s pairing needs %s (n_series %lld, n_draws %lld)",
            r->pairing == HHMM_PAIR_ZIP ? "ZIP" : "BLOCK",
            r->pairing == HHMM_PAIR_ZIP ? "n_series == n_draws" : "n_draws a multiple of n_series",
            (long long)d.n_series, (long long)w.n_draws);
    REQUIRE(d.T_max >= 1, "T_max must be >= 1 (int<lower=1> T)");
    /* kernels address rows as uniform base + 32-bit lane offset (8-byte elements) */
    REQUIRE(npairs(r) <= (int64_t(1) << 28) && d.n_series <= (int64_t(1) << 28) && w.n_draws <= (int64_t(1) << 28),
            "at most 2^28 pairs / series / draws per call (split larger batches)");
    REQUIRE(d.K >= 1, "K must be >= 1 (int<lower=1> K)");
    const int m = r->model;
    if (is_discrete(m))
        REQUIRE(d.L >= 1 && d.x_int, "model %d needs L >= 1 and x_int", m);
    if (m == HHMM_MODEL_HMM_GAUSS || is_iohmm(m))
        REQUIRE(d.x_real, "model %d needs x_real", m);
    if (is_iohmm(m))
        REQUIRE(d.M >= 1 && d.u, "IOHMM needs M >= 1 and u_tm");
    if (m == HHMM_MODEL_HMM_MULTINOM_SEMISUP)
        REQUIRE(d.G >= 1 && d.g, "semisup needs G >= 1 and g");
    if (m == HHMM_MODEL_TAYAL || m == HHMM_MODEL_TAYAL_LITE) {
        REQUIRE(d.K == 4, "the Tayal model is the K = 4 flattened HHMM (got K = %d)", d.K);
        REQUIRE(d.sign && w.p_11 && w.A_row && w.phi_k, "tayal needs sign, p_11, A_row, phi_k");
    }
    if (m == HHMM_MODEL_TAYAL_LITE)
        REQUIRE(d.T_oos_max >= 1 && d.x_oos && d.sign_oos, "tayal-lite needs T_oos_max, x_oos, sign_oos");
    if (m == HHMM_MODEL_HMM_GAUSS)
        REQUIRE(w.p_1k && w.A_ij && w.mu_k && w.sigma_k, "hmm-gauss needs p_1k, A_ij, mu_k, sigma_k");
    if (m == HHMM_MODEL_HMM_MULTINOM || m == HHMM_MODEL_HMM_MULTINOM_SEMISUP)
        REQUIRE(w.p_1k && w.A_ij && w.phi_k, "multinomial HMM needs p_1k, A_ij, phi_k");
    if (m == HHMM_MODEL_IOHMM_REG)
        REQUIRE(w.p_1k && w.w_km && w.b_km && w.s_k, "iohmm-reg needs p_1k, w_km, b_km, s_k");
    if (m == HHMM_MODEL_IOHMM_MIX || m == HHMM_MODEL_IOHMM_HMIX || m == HHMM_MODEL_IOHMM_HMIX_LITE)
        REQUIRE(d.L >= 1 && w.p_1k && w.w_km && w.lambda_kl && w.mu_kl && w.s_kl,
                "iohmm-mix needs L, p_1k, w_km, lambda_kl, mu_kl, s_kl");

    const uint32_t avail = available_outputs(m);
    REQUIRE((r->outputs & ~avail) == 0, "outputs 0x%x not declared by model %d (available 0x%x)",
            r->outputs & ~avail, m, avail);
    REQUIRE(r->outputs != 0, "no outputs requested");
    static const hhmm_result none{};
    const hhmm_result *oo = o ? o : &none;
    struct {
        uint32_t bit;
        const void *ptr;
        const char *name;
    } outs[] = {{HHMM_OUT_LOGLIK, oo->loglik, "loglik"},
                {HHMM_OUT_UNALPHA, oo->unalpha_tk, "unalpha_tk"},
                {HHMM_OUT_ALPHA, oo->alpha_tk, "alpha_tk"},
                {HHMM_OUT_UNBETA, oo->unbeta_tk, "unbeta_tk"},
                {HHMM_OUT_BETA, oo->beta_tk, "beta_tk"},
                {HHMM_OUT_UNGAMMA, oo->ungamma_tk, "ungamma_tk"},
                {HHMM_OUT_GAMMA, oo->gamma_tk, "gamma_tk"},
                {HHMM_OUT_ZSTAR, oo->zstar_t, "zstar_t"},
                {HHMM_OUT_LOGP_ZSTAR, oo->logp_zstar, "logp_zstar"},
                {HHMM_OUT_OBLIK_TK, oo->oblik_tk, "oblik_tk"},
                {HHMM_OUT_OBLIK_T, oo->oblik_t, "oblik_t"},
                {HHMM_OUT_FFBS, oo->z_ffbs, "z_ffbs"},
                {HHMM_OUT_ALPHA_OOS, oo->alpha_tk_oos, "alpha_tk_oos"},
                {HHMM_OUT_UNALPHA_OOS, oo->unalpha_tk_oos, "unalpha_tk_oos"},
                {HHMM_OUT_LOGA, oo->logA_ij, "logA_ij"},
                {HHMM_OUT_HATPI, oo->hatpi_tk, "hatpi_tk"},
                {HHMM_OUT_HATZ, oo->hatz_t, "hatz_t"},
                {HHMM_OUT_HATL, oo->hatl_t, "hatl_t"},
                {HHMM_OUT_HATX, oo->hatx_t, "hatx_t"}};
    if (o)
        for (auto &e : outs)
            REQUIRE(!(r->outputs & e.bit) || e.ptr, "output %s requested but its pointer is NULL", e.name);
    if (r->outputs & HHMM_OUT_FFBS)
        REQUIRE(r->ffbs_u, "FFBS needs ffbs_u");
    if (r->outputs & (HHMM_OUT_HATZ | HHMM_OUT_HATL | HHMM_OUT_HATX))
        REQUIRE(r->hat_rand, "hatz_t / hatl_t / hatx_t need hat_rand");

    if (host) {
        const int64_t N = d.n_series;
        const int Tm = d.T_max;
        if (d.T)
            for (int64_t n = 0; n < N; ++n)
                REQUIRE(d.T[n] >= 1 && d.T[n] <= Tm, "T[%lld] = %d outside 1..T_max=%d", (long long)n, d.T[n], Tm);
        auto len = [&](int64_t n) { return d.T ? d.T[n] : Tm; };
        /* the fast time-major scan first; the n-major loops below only run to
         * name the first offender when it found one */
        if (is_discrete(m) && any_out_of_range(d.x_int, N, Tm, d.T, 1, d.L))
            for (int64_t n = 0; n < N; ++n)
                for (int t = 0; t < len(n); ++t) {
                    const int32_t v = d.x_int[n + N * (int64_t)t];
                    REQUIRE(v >= 1 && v <= d.L, "x[%lld, %d] = %d outside 1..L=%d", (long long)n, t + 1, v, d.L);
                }
        if (m == HHMM_MODEL_HMM_MULTINOM_SEMISUP && any_out_of_range(d.g, N, Tm, d.T, 1, d.G))
            for (int64_t n = 0; n < N; ++n)
                for (int t = 0; t < len(n); ++t) {
                    const int32_t v = d.g[n + N * (int64_t)t];
                    REQUIRE(v >= 1 && v <= d.G, "g[%lld, %d] = %d outside 1..G=%d", (long long)n, t + 1, v, d.G);
                }
        if ((m == HHMM_MODEL_TAYAL || m == HHMM_MODEL_TAYAL_LITE) && any_out_of_range(d.sign, N, Tm, d.T, 1, 2))
            for (int64_t n = 0; n < N; ++n)
                for (int t = 0; t < len(n); ++t) {
                    const int32_t v = d.sign[n + N * (int64_t)t];
                    REQUIRE(v == 1 || v == 2, "sign[%lld, %d] = %d outside 1..2", (long long)n, t + 1, v);
                }
        if (m == HHMM_MODEL_TAYAL_LITE) {
            for (int64_t n = 0; n < N; ++n) {
                const int To = d.T_oos ? d.T_oos[n] : d.T_oos_max;
                REQUIRE(To >= 1 && To <= d.T_oos_max, "T_oos[%lld] = %d outside 1..T_oos_max", (long long)n, To);
                for (int t = 0; t < To; ++t) {
                    const int32_t v = d.x_oos[n + N * (int64_t)t];
                    const int32_t sg = d.sign_oos[n + N * (int64_t)t];
                    REQUIRE(v >= 1 && v <= d.L, "x_oos[%lld, %d] = %d outside 1..L", (long long)n, t + 1, v);
                    REQUIRE(sg == 1 || sg == 2, "sign_oos[%lld, %d] = %d outside 1..2", (long long)n, t + 1, sg);
                }
            }
        }
        if (m == HHMM_MODEL_HMM_GAUSS)
            for (int64_t i = 0; i < w.n_draws * d.K; ++i)
                REQUIRE(w.sigma_k[i] > 0.0, "sigma_k must be > 0 (real<lower=0.0001>)");
    }
    return HHMM_OK;
}

static hhmm_status validate(const hhmm_request *r, const hhmm_result *o, bool host)
{
    REQUIRE(r && o, "request and result must be non-NULL");
    return validate_impl(r, o, host);
}

hhmm_status hip_fail(hipError_t e, const char *what)
{
    set_error("%s: %s", what, hipGetErrorString(e));
    return (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) ? HHMM_ERR_OUT_OF_MEMORY : HHMM_ERR_HIP;
}

hhmm_status check_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        set_error("no HIP device visible: libhhmm has no CPU path (gfx950 required)");
        return HHMM_ERR_NO_DEVICE;
    }
    return HHMM_OK;
}

static hhmm_status check_arch(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return hip_fail(hipGetLastError(), "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s, this build targets gfx950", dev, prop.gcnArchName);
        return HHMM_ERR_NO_DEVICE;
    }
    return HHMM_OK;
}

/* ---------------- device set (hhmm_init / hhmm_init_devices) ---------------- */
struct DevSet {
    std::mutex mu;
    std::vector<int> devs; /* ordinals HHMM_DEVICE_SET shards over (repeats allowed); empty: {0} */
};
static DevSet &devset()
{
    static DevSet d;
    return d;
}
static std::vector<int> device_set()
{
    std::lock_guard<std::mutex> g(devset().mu);
    return devset().devs.empty() ? std::vector<int>{0} : devset().devs;
}

/* ---------------- the R path: a pipelined host request ----------------
 * hhmm_run's caller hands over pageable host arrays (R's REAL() buffers,
 * SURVEY §8b).  A device's shard is split into chunks of series (or draws),
 * and chunk i's upload and kernels overlap chunk i-1's download: per device
 * three non-blocking streams (upload, compute, download), two slots of
 * device buffers and two pinned staging slots per direction.  The host thread
 * gathers chunk i's input rows into a pinned slot (threads over rows), the
 * upload stream DMAs the slot to the device in one copy, the compute stream
 * runs the chunk's sub-request, the download stream DMAs its outputs and
 * pair_status into the other pinned slot in one copy, and the host thread
 * scatters chunk i-1's rows into the caller's arrays meanwhile.  Every array
 * of a chunk sits at the same offset in its device slot and its pinned slot,
 * so each direction is one DMA per chunk. */

struct HostPool { /* pinned staging blocks, reused across calls (hhmm_shutdown frees them) */
    std::mutex mu;
    std::multimap<size_t, void *> free_blocks;
    std::map<void *, size_t> live;
};
static HostPool &host_pool()
{
    static HostPool p;
    return p;
}
static void *host_get(size_t bytes)
{
    bytes = (std::max<size_t>(bytes, 4096) + 4095) & ~(size_t)4095;
    HostPool &p = host_pool();
    {
        std::lock_guard<std::mutex> g(p.mu);
        auto it = p.free_blocks.lower_bound(bytes);
        if (it != p.free_blocks.end() && it->first <= bytes + bytes / 4) {
            void *ptr = it->second;
            p.live[ptr] = it->first;
            p.free_blocks.erase(it);
            return ptr;
        }
    }
    void *ptr = nullptr;
    if (hipHostMalloc(&ptr, bytes, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::lock_guard<std::mutex> g(p.mu);
    p.live[ptr] = bytes;
    return ptr;
}
static void host_put(void *ptr)
{
    if (!ptr)
        return;
    HostPool &p = host_pool();
    std::lock_guard<std::mutex> g(p.mu);
    auto it = p.live.find(ptr);
    if (it == p.live.end())
        return;
    p.free_blocks.emplace(it->second, ptr);
    p.live.erase(it);
}
static void host_release_all()
{
    HostPool &p = host_pool();
    std::lock_guard<std::mutex> g(p.mu);
    for (auto &kv : p.free_blocks)
        (void)hipHostFree(kv.second);
    p.free_blocks.clear();
}

struct PipeStreams {
    std::mutex mu;
    std::map<int, std::vector<hipStream_t>> by_dev; /* upload, compute, download */
};
static PipeStreams &pipe_streams()
{
    static PipeStreams s;
    return s;
}
static hhmm_status get_pipe_streams(int dev, hipStream_t (&st)[3])
{
    PipeStreams &ps = pipe_streams();
    std::lock_guard<std::mutex> g(ps.mu);
    auto it = ps.by_dev.find(dev);
    if (it == ps.by_dev.end()) {
        std::vector<hipStream_t> v(3, nullptr);
        for (auto &x : v)
            if (hipStreamCreateWithFlags(&x, hipStreamNonBlocking) != hipSuccess) {
                set_error("device %d: stream creation failed", dev);
                return HHMM_ERR_HIP;
            }
        it = ps.by_dev.emplace(dev, v).first;
    }
    for (int i = 0; i < 3; ++i)
        st[i] = it->second[(size_t)i];
    return HHMM_OK;
}

/* The whole request runs no parallel scan over T.  Only then may it be cut
 * into chunks or ranges: with kSequentialFlags pinned they take the same
 * sequential recursions, and the outputs are bit-identical to one device call. */
static bool runs_sequentially(const hhmm_request *req)
{
    const hhmm_data &d = req->data;
    const int64_t Pw = npairs(req);
    return scan_plan(req->model, d.K, d.T_max, Pw, req->outputs, (uint32_t)req->flags).cl == 0 &&
           vscan_chunks(req->model, d.K, req->model == HHMM_MODEL_TAYAL_LITE ? d.T_oos_max : d.T_max, Pw, req->outputs,
                        (uint32_t)req->flags) == 0;
}
constexpr int32_t kSequentialFlags = (int32_t)(HHMM_FLAG_SCAN_OFF | HHMM_FLAG_VIT_SCAN_OFF);

/* Chunks of a device shard: about kChunkBytes of staged traffic each, with at
 * least kChunkMinPairs pairs (256 waves) so a chunk's kernels still fill the
 * chip, and only where the request runs_sequentially (pin_flags: the caller
 * pins kSequentialFlags).  HHMM_FLAG_HOST_CHUNKS(n) asks for n chunks. */
constexpr size_t kChunkBytes = (size_t)512 << 20;
constexpr int64_t kChunkMinPairs = 16384;

static int64_t choose_chunks(const hhmm_request *req, const std::vector<ArrayDesc> &arrays, const Shard &sh,
                             bool ragged, bool &pin_flags)
{
    pin_flags = false;
    if (!runs_sequentially(req))
        return 1;
    const int64_t forced = (int64_t)(((uint32_t)req->flags >> 20) & 0xffu);
    size_t bytes = 0; /* staged bytes of the shard, both directions */
    for (const ArrayDesc &a : arrays)
        bytes += shard_bytes(a, sh) * ((a.output && ragged) ? 2 : 1);
    const int64_t P = sh.cnt[PAIRS];
    int64_t n = forced > 0 ? forced : (int64_t)((bytes + kChunkBytes - 1) / kChunkBytes);
    if (forced == 0)
        n = std::min<int64_t>(n, std::max<int64_t>(1, P / kChunkMinPairs));
    n = std::max<int64_t>(1, n);
    pin_flags = n > 1;
    return n;
}

/* The tail of a device path whose launch (ls) or HIP call (e) failed.  A
 * failed launch may follow one that is still running: drain() waits for the
 * request's streams before cleanup() hands its pooled buffers to another
 * request; a sticky device error from an earlier fault is reported beside the
 * launch error instead of being buried under it. */
template <class Drain, class Cleanup>
static hhmm_status fail_drained(hhmm_status ls, hipError_t e, Drain drain, Cleanup cleanup, const char *what,
                                const char *streams)
{
    const std::string first = hhmm_last_error();
    const hipError_t d = drain();
    cleanup();
    if (ls == HHMM_OK)
        return hip_fail(e, what);
    if (d != hipSuccess)
        set_error("%s; draining the request's %s then failed: %s", first.c_str(), streams, hipGetErrorString(d));
    return ls;
}

/* Runs one shard of a host request on the current device (the pipeline
 * above).  status: the caller's [P] host array, written at the shard's pairs;
 * *failures counts them. */
static hhmm_status run_on_device(const hhmm_request *req, hhmm_result *res, const Shard &sh, int32_t *status,
                                 int64_t *failures)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return hip_fail(e, "hipGetDevice");
    hhmm_request dreq = *req;
    hhmm_result dres = *res;
    dres.pair_status = nullptr;
    std::vector<ArrayDesc> arrays;
    describe(req, res, &dreq, &dres, arrays);
    const bool ragged = req->data.T != nullptr || req->data.T_oos != nullptr;
    bool pin = false;
    const int64_t nch = choose_chunks(req, arrays, sh, ragged, pin);
    const std::vector<Shard> chunks = split_shard(req, sh, nch);
    std::vector<ChunkLayout> lay;
    size_t slot_bytes = 0, in_bytes = 0, out_bytes = 0, wsb = 0;
    for (const Shard &c : chunks) {
        lay.push_back(chunk_layout(req, arrays, c, ragged));
        const ChunkLayout &L = lay.back();
        if (L.P < 1) {
            set_error("internal: shard describes no pairs");
            return HHMM_ERR_INVALID_ARGUMENT;
        }
        if (!chunk_pairs_agree(req, c, L)) {
            set_error("internal: a chunk stages %lld pairs for a sub-request of %lld",
                      (long long)chunk_staged_pairs(req, c), (long long)L.P);
            return HHMM_ERR_INVALID_ARGUMENT;
        }
        slot_bytes = std::max(slot_bytes, L.total);
        in_bytes = std::max(in_bytes, L.in_end);
        out_bytes = std::max(out_bytes, L.total - L.out_begin);
        wsb = std::max(wsb, workspace_bytes(dreq.model, dreq.data.K, dreq.data.L, dreq.data.T_max,
                                            dreq.data.T_oos_max, L.P, dreq.outputs, (uint32_t)dreq.flags,
                                            c.cnt[SERIES], dreq.pairing));
    }
    if (pin)
        dreq.flags |= kSequentialFlags;
    const int nslot = chunks.size() > 1 ? 2 : 1;
    hipStream_t st[3];
    hhmm_status s = get_pipe_streams(dev, st);
    if (s != HHMM_OK)
        return s;
    void *dslot[2] = {nullptr, nullptr}, *hin[2] = {nullptr, nullptr}, *hout[2] = {nullptr, nullptr};
    void *ws = nullptr;
    hipEvent_t ev[3][2] = {}; /* uploaded, computed, downloaded -- per slot */
    auto cleanup = [&]() {
        for (int k = 0; k < 2; ++k) {
            pool_put(dslot[k]);
            host_put(hin[k]);
            host_put(hout[k]);
            for (int j = 0; j < 3; ++j)
                if (ev[j][k])
                    (void)hipEventDestroy(ev[j][k]);
        }
        pool_put(ws);
    };
    auto drain = [&]() { /* every stream of this request, the side stream included */
        hipError_t r = hipSuccess;
        for (int j = 0; j < 3; ++j) {
            const hipError_t q = (j == 1) ? sync_request(st[1]) : hipStreamSynchronize(st[j]);
            if (r == hipSuccess)
                r = q;
        }
        return r;
    };
    for (int k = 0; k < nslot; ++k) {
        dslot[k] = pool_get(dev, slot_bytes);
        hin[k] = host_get(in_bytes);
        hout[k] = host_get(out_bytes);
        for (int j = 0; j < 3; ++j)
            if (hipEventCreateWithFlags(&ev[j][k], hipEventDisableTiming) != hipSuccess)
                ev[j][k] = nullptr;
        if (!dslot[k] || !hin[k] || !hout[k] || !ev[0][k] || !ev[1][k] || !ev[2][k]) {
            cleanup();
            set_error("device %d: allocation of the host pipeline's buffers failed (%zu device, %zu + %zu pinned bytes)",
                      dev, slot_bytes, in_bytes, out_bytes);
            return HHMM_ERR_OUT_OF_MEMORY;
        }
    }
    ws = pool_get(dev, wsb);
    if (!ws) {
        cleanup();
        set_error("device %d: workspace allocation of %zu bytes failed", dev, wsb);
        return HHMM_ERR_OUT_OF_MEMORY;
    }

    const int64_t Pw = npairs(req);
    int64_t fails = 0;
    hhmm_status ls = HHMM_OK;
    const size_t n = chunks.size();
    for (size_t i = 0; i < n && ls == HHMM_OK; ++i) {
        const int k = (int)(i % (size_t)nslot);
        const ChunkLayout &L = lay[i];
        if (i >= (size_t)nslot && (e = hipEventSynchronize(ev[0][k])) != hipSuccess) /* pinned in-slot free */
            break;
        gather_chunk(arrays, L, hin[k]);
        if (i >= (size_t)nslot && (e = hipStreamWaitEvent(st[0], ev[2][k], 0)) != hipSuccess) /* device slot free */
            break;
        if ((e = hipMemcpyAsync(dslot[k], hin[k], L.in_end, hipMemcpyHostToDevice, st[0])) != hipSuccess ||
            (e = hipEventRecord(ev[0][k], st[0])) != hipSuccess || (e = hipStreamWaitEvent(st[1], ev[0][k], 0)) !=
                                                                         hipSuccess ||
            (e = hipMemsetAsync((char *)dslot[k] + L.status_off, 0, (size_t)L.P * sizeof(int32_t), st[1])) !=
                hipSuccess)
            break;
        hhmm_request cr;
        hhmm_result cq;
        bind_chunk(arrays, L, dslot[k], dreq, dres, cr, cq);
        ls = launch_all(&cr, &cq, L.P, ws, st[1]);
        if (ls != HHMM_OK)
            break;
        if ((e = hipEventRecord(ev[1][k], st[1])) != hipSuccess || (e = hipStreamWaitEvent(st[2], ev[1][k], 0)) !=
                                                                        hipSuccess ||
            (e = hipMemcpyAsync(hout[k], (char *)dslot[k] + L.out_begin, L.total - L.out_begin,
                                hipMemcpyDeviceToHost, st[2])) != hipSuccess ||
            (e = hipEventRecord(ev[2][k], st[2])) != hipSuccess)
            break;
        if (i >= 1) { /* the previous chunk's outputs, while this one uploads and runs */
            const int kp = (int)((i - 1) % (size_t)nslot);
            if ((e = hipEventSynchronize(ev[2][kp])) != hipSuccess)
                break;
            fails += scatter_chunk(arrays, lay[i - 1], hout[kp], status, Pw);
        }
    }
    if (ls != HHMM_OK || e != hipSuccess)
        return fail_drained(ls, e, drain, cleanup, "host pipeline (copy or kernel execution)", "streams");
    e = drain();
    if (e != hipSuccess) {
        cleanup();
        return hip_fail(e, "kernel execution");
    }
    fails += scatter_chunk(arrays, lay[n - 1], hout[(n - 1) % (size_t)nslot], status, Pw);
    cleanup();
    *failures = fails;
    return HHMM_OK;
}

/* Item i of n on device devs[i], each on a host thread of its own
 * (run_parallel); run(i) finds that device current.  The thread-local error
 * text of a failing item is carried to the caller's thread, and the first
 * failing item's status returns, its text behind "`what` i (device d): " (no
 * prefix where `what` is NULL). */
static hhmm_status run_per_device(const std::vector<int> &devs, size_t n, const char *what,
                                  const std::function<hhmm_status(size_t)> &run)
{
    std::vector<hhmm_status> st(n, HHMM_OK);
    std::vector<std::string> msg(n);
    run_parallel(n, [&](size_t i) {
        const hipError_t e = hipSetDevice(devs[i]);
        st[i] = e != hipSuccess ? hip_fail(e, "hipSetDevice") : run(i);
        if (st[i] != HHMM_OK)
            msg[i] = hhmm_last_error();
    });
    for (size_t i = 0; i < n; ++i)
        if (st[i] != HHMM_OK) {
            if (what)
                set_error("%s %zu (device %d): %s", what, i, devs[i], msg[i].c_str());
            else
                set_error("%s", msg[i].c_str());
            return st[i];
        }
    return HHMM_OK;
}

/* The end of a host request that ran: the pair statuses to the caller's
 * array (optional), and the warning when any pair failed. */
static hhmm_status report_pairs(const std::vector<int32_t> &status, int64_t P, int32_t *pair_status,
                                const std::vector<int64_t> &fails)
{
    if (pair_status)
        memcpy(pair_status, status.data(), (size_t)P * sizeof(int32_t));
    int64_t failures = 0;
    for (int64_t f : fails)
        failures += f;
    if (failures) {
        set_error("%lld pair(s) hit an unset Viterbi back-pointer (Stan would throw)", (long long)failures);
        return HHMM_WARN_PAIR_FAILURES;
    }
    return HHMM_OK;
}

/* HHMM_DEVICE_SET: one host thread per shard, each on its device of the set
 * (hhmm_init / hhmm_init_devices), writing its slices of the caller's
 * outputs; the first failing shard's error is returned (device
 * set {GPU 0..7}, one host thread per GPU; §8e: contiguous series ranges). */
static hhmm_status run_sharded(const hhmm_request *req, hhmm_result *res)
{
    const std::vector<int> devs = device_set();
    const std::vector<Shard> shards = make_shards(req, (int)devs.size());
    const int64_t P = npairs(req);
    std::vector<int32_t> status((size_t)P, 0);
    std::vector<int64_t> fails(shards.size(), 0);
    int cur = 0;
    (void)hipGetDevice(&cur);
    const hhmm_status s = run_per_device(devs, shards.size(), "shard", [&](size_t i) {
        return run_on_device(req, res, shards[i], status.data(), &fails[i]);
    });
    (void)hipSetDevice(cur);
    if (s != HHMM_OK)
        return s;
    return report_pairs(status, P, res->pair_status, fails);
}

/* ---------------- hhmm_run_summary: run, reduce over draws, download the summaries ----------------
 * Ranges of series run one after the other on the device's compute stream:
 * gather + upload the range's inputs, the request's kernels into a pooled
 * device slot (the per-draw [P, T, ...] arrays live only there), one summary
 * launch per reduced output into a pooled summary buffer, then one download of
 * that buffer, the [P] outputs and pair_status.  What returns is Q/S of what
 * hhmm_run moves, so the ranges are not overlapped. */
constexpr uint32_t kSumAllBits = (1u << 19) - 1;
constexpr uint32_t kSumPairBits = HHMM_OUT_LOGLIK | HHMM_OUT_LOGP_ZSTAR; /* [P]: to `pairs`, not reduced */
constexpr uint32_t kSumStepBits = kSumAllBits & ~kSumPairBits;
constexpr uint32_t kSumKAxisBits = HHMM_OUT_UNALPHA | HHMM_OUT_ALPHA | HHMM_OUT_UNBETA | HHMM_OUT_BETA |
                                   HHMM_OUT_UNGAMMA | HHMM_OUT_GAMMA | HHMM_OUT_OBLIK_TK | HHMM_OUT_ALPHA_OOS |
                                   HHMM_OUT_UNALPHA_OOS | HHMM_OUT_LOGA | HHMM_OUT_HATPI;
constexpr size_t kSummaryBudget = (size_t)8 << 30; /* device bytes of one range (and at most 3/4 of what is free) */

/* The hhmm_result field of a per-step output bit. */
static size_t sum_field(int bit, bool &i32)
{
    i32 = false;
    switch (1u << bit) {
    case HHMM_OUT_UNALPHA: return offsetof(hhmm_result, unalpha_tk);
    case HHMM_OUT_ALPHA: return offsetof(hhmm_result, alpha_tk);
    case HHMM_OUT_UNBETA: return offsetof(hhmm_result, unbeta_tk);
    case HHMM_OUT_BETA: return offsetof(hhmm_result, beta_tk);
    case HHMM_OUT_UNGAMMA: return offsetof(hhmm_result, ungamma_tk);
    case HHMM_OUT_GAMMA: return offsetof(hhmm_result, gamma_tk);
    case HHMM_OUT_ZSTAR: i32 = true; return offsetof(hhmm_result, zstar_t);
    case HHMM_OUT_OBLIK_TK: return offsetof(hhmm_result, oblik_tk);
    case HHMM_OUT_OBLIK_T: return offsetof(hhmm_result, oblik_t);
    case HHMM_OUT_FFBS: i32 = true; return offsetof(hhmm_result, z_ffbs);
    case HHMM_OUT_ALPHA_OOS: return offsetof(hhmm_result, alpha_tk_oos);
    case HHMM_OUT_UNALPHA_OOS: return offsetof(hhmm_result, unalpha_tk_oos);
    case HHMM_OUT_LOGA: return offsetof(hhmm_result, logA_ij);
    case HHMM_OUT_HATPI: return offsetof(hhmm_result, hatpi_tk);
    case HHMM_OUT_HATZ: i32 = true; return offsetof(hhmm_result, hatz_t);
    case HHMM_OUT_HATL: i32 = true; return offsetof(hhmm_result, hatl_t);
    case HHMM_OUT_HATX: return offsetof(hhmm_result, hatx_t);
    default: return (size_t)-1;
    }
}
static bool sum_uses_oos(const hhmm_request *r, int bit)
{
    const uint32_t b = 1u << bit;
    return (b & (HHMM_OUT_ALPHA_OOS | HHMM_OUT_UNALPHA_OOS)) ||
           (b == HHMM_OUT_ZSTAR && r->model == HHMM_MODEL_TAYAL_LITE);
}
static size_t sum_T(const hhmm_request *r, int bit)
{
    return (size_t)(sum_uses_oos(r, bit) ? r->data.T_oos_max : r->data.T_max);
}
static size_t sum_K(const hhmm_request *r, int bit) { return ((1u << bit) & kSumKAxisBits) ? (size_t)r->data.K : 1; }

/* Where each summary of a range of Nc series sits in the range's summary buffer. */
struct SumPlan {
    size_t qoff[32], aoff[32], total;
};
static SumPlan sum_plan(const hhmm_request *r, const hhmm_summary_spec *sp, int64_t Nc)
{
    SumPlan p{};
    size_t o = 0;
    for (int b = 0; b < 32; ++b) {
        if (!((sp->summarise >> b) & 1u))
            continue;
        const size_t cells = (size_t)Nc * sum_T(r, b);
        p.qoff[b] = o;
        o += (sizeof(double) * cells * sum_K(r, b) * (size_t)sp->n_probs + 255) & ~(size_t)255;
        if ((sp->argmax >> b) & 1u) {
            p.aoff[b] = o;
            o += (sizeof(int32_t) * cells + 255) & ~(size_t)255;
        }
    }
    p.total = o;
    return p;
}

/* Series [a0, a1) of the request on the current device.  `full`: the result
 * describe() sees (the caller's [P] pointers; placeholders, never
 * dereferenced, for the per-step outputs, which exist on the device only). */
static hhmm_status run_summary_on_device(const hhmm_request *req, const hhmm_summary_spec *spec,
                                         const hhmm_result *full, hhmm_summary_result *out, int64_t a0, int64_t a1,
                                         bool split_outside, int32_t *status, int64_t *failures)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return hip_fail(e, "hipGetDevice");
    hhmm_request dreq = *req;
    hhmm_result dres = *full;
    dres.pair_status = nullptr;
    std::vector<ArrayDesc> arrays;
    describe(req, full, &dreq, &dres, arrays);
    const hhmm_data &d = req->data;
    const int64_t N = d.n_series;
    const bool seq = runs_sequentially(req);
    const int64_t forced = (int64_t)(((uint32_t)req->flags >> 20) & 0xffu);
    size_t freeb = 0, totalb = 0;
    if ((e = hipMemGetInfo(&freeb, &totalb)) != hipSuccess)
        return hip_fail(e, "hipMemGetInfo");
    const size_t budget = std::min(kSummaryBudget, freeb / 4 * 3);
    auto ws_of = [&](const Shard &c, int64_t P) {
        return workspace_bytes(dreq.model, d.K, d.L, d.T_max, d.T_oos_max, P, dreq.outputs, (uint32_t)dreq.flags,
                               c.cnt[SERIES], dreq.pairing);
    };
    auto worst = [&](const std::vector<Shard> &v) {
        size_t w = 0;
        for (const Shard &c : v) {
            const ChunkLayout L = chunk_layout(req, arrays, c, false);
            w = std::max(w, L.total + ws_of(c, L.P) + sum_plan(req, spec, c.cnt[SERIES]).total);
        }
        return w;
    };
    int64_t nr = (seq && forced > 0) ? std::min(forced, a1 - a0) : 1;
    std::vector<Shard> ranges = series_ranges(req, a0, a1, nr);
    if (forced == 0 || !seq) {
        for (;;) {
            const size_t w = worst(ranges);
            if (w <= budget)
                break;
            if (!seq) {
                set_error("the request runs a parallel scan over T and stays one range, which needs %zu device bytes "
                          "(budget %zu)", w, budget);
                return HHMM_ERR_OUT_OF_MEMORY;
            }
            if (nr >= a1 - a0) {
                set_error("a single series needs %zu device bytes of per-draw outputs and workspace, over the "
                          "budget of %zu: nothing smaller to split into", w, budget);
                return HHMM_ERR_OUT_OF_MEMORY;
            }
            nr = std::min(a1 - a0, std::max(nr + 1, nr + nr / 4));
            ranges = series_ranges(req, a0, a1, nr);
        }
    }
    if (seq && (ranges.size() > 1 || split_outside))
        dreq.flags |= kSequentialFlags;

    /* the [P] outputs among `arrays`, and their place behind the summaries in the download slot */
    std::vector<size_t> pair_arrays;
    for (size_t i = 0; i < arrays.size(); ++i)
        if (arrays[i].output && (arrays[i].field == offsetof(hhmm_result, loglik) ||
                                 arrays[i].field == offsetof(hhmm_result, logp_zstar)))
            pair_arrays.push_back(i);
    std::vector<ChunkLayout> lay;
    std::vector<SumPlan> plans;
    size_t slot_bytes = 0, in_bytes = 0, sum_bytes = 0, host_bytes = 0, wsb = 0;
    for (const Shard &c : ranges) {
        lay.push_back(chunk_layout(req, arrays, c, false));
        plans.push_back(sum_plan(req, spec, c.cnt[SERIES]));
        const ChunkLayout &L = lay.back();
        if (L.P < 1 || !chunk_pairs_agree(req, c, L) || L.P % c.cnt[SERIES] != 0 ||
            L.P / c.cnt[SERIES] > HHMM_SUMMARY_MAX_DRAWS) {
            set_error("internal: a summary range of %lld series describes %lld pairs", (long long)c.cnt[SERIES],
                      (long long)L.P);
            return HHMM_ERR_INVALID_ARGUMENT;
        }
        slot_bytes = std::max(slot_bytes, L.total);
        in_bytes = std::max(in_bytes, L.in_end);
        sum_bytes = std::max(sum_bytes, plans.back().total);
        host_bytes = std::max(host_bytes, plans.back().total + (pair_arrays.size() * 8 + 4) * (size_t)L.P + 1024);
        wsb = std::max(wsb, ws_of(c, L.P));
    }
    hipStream_t pst[3];
    hhmm_status s = get_pipe_streams(dev, pst);
    if (s != HHMM_OK)
        return s;
    const hipStream_t st = pst[1];
    void *dslot = pool_get(dev, slot_bytes), *dsum = pool_get(dev, sum_bytes), *ws = pool_get(dev, wsb);
    void *hin = host_get(in_bytes), *hout = host_get(host_bytes);
    auto cleanup = [&]() {
        pool_put(dslot);
        pool_put(dsum);
        pool_put(ws);
        host_put(hin);
        host_put(hout);
    };
    if (!dslot || !dsum || !ws || !hin || !hout) {
        cleanup();
        set_error("device %d: allocation of a summary range's buffers failed (%zu + %zu + %zu device, %zu + %zu "
                  "pinned bytes)", dev, slot_bytes, sum_bytes, wsb, in_bytes, host_bytes);
        return HHMM_ERR_OUT_OF_MEMORY;
    }
    const bool ragged = d.T != nullptr || d.T_oos != nullptr;
    const size_t Q = (size_t)spec->n_probs;
    /* the caller's summary arrays <-> the range's packed [Nc, ...] copies in hout */
    auto move_summaries = [&](const Shard &c, const SumPlan &pl, bool to_host_arrays) {
        const size_t Nc = (size_t)c.cnt[SERIES], a = (size_t)c.off[SERIES];
        for (int b = 0; b < 32; ++b) {
            if (!((spec->summarise >> b) & 1u))
                continue;
            const size_t rows = sum_T(req, b) * sum_K(req, b) * Q;
            char *hq = (char *)(out->quantiles[b] + a), *pq = (char *)hout + pl.qoff[b];
            if (to_host_arrays)
                par_copy_rows(hq, (size_t)N * 8, pq, Nc * 8, Nc * 8, rows);
            else
                par_copy_rows(pq, Nc * 8, hq, (size_t)N * 8, Nc * 8, rows);
            if ((spec->argmax >> b) & 1u) {
                char *ha = (char *)(out->argmax[b] + a), *pa = (char *)hout + pl.aoff[b];
                if (to_host_arrays)
                    par_copy_rows(ha, (size_t)N * 4, pa, Nc * 4, Nc * 4, sum_T(req, b));
                else
                    par_copy_rows(pa, Nc * 4, ha, (size_t)N * 4, Nc * 4, sum_T(req, b));
            }
        }
    };
    int64_t fails = 0;
    hhmm_status ls = HHMM_OK;
    for (size_t i = 0; i < ranges.size(); ++i) {
        const ChunkLayout &L = lay[i];
        const SumPlan &pl = plans[i];
        const Shard &c = ranges[i];
        gather_chunk(arrays, L, hin);
        if ((e = hipMemcpyAsync(dslot, hin, L.in_end, hipMemcpyHostToDevice, st)) != hipSuccess)
            break;
        if (ragged) { /* steps past a series' end keep the caller's fill: they travel up and back */
            move_summaries(c, pl, false);
            if ((e = hipMemcpyAsync(dsum, hout, pl.total, hipMemcpyHostToDevice, st)) != hipSuccess)
                break;
        }
        if ((e = hipMemsetAsync((char *)dslot + L.status_off, 0, (size_t)L.P * sizeof(int32_t), st)) != hipSuccess)
            break;
        hhmm_request cr;
        hhmm_result cq;
        bind_chunk(arrays, L, dslot, dreq, dres, cr, cq);
        if ((ls = launch_all(&cr, &cq, L.P, ws, st)) != HHMM_OK)
            break;
        for (int b = 0; b < 32 && ls == HHMM_OK; ++b) {
            if (!((spec->summarise >> b) & 1u))
                continue;
            bool i32 = false;
            const size_t fo = sum_field(b, i32);
            hhmm_summary_request sr{};
            sr.n_series = c.cnt[SERIES];
            sr.n_draws = L.P / c.cnt[SERIES];
            sr.T_max = (int32_t)sum_T(req, b);
            sr.K = (int32_t)sum_K(req, b);
            sr.T = sum_uses_oos(req, b) ? cr.data.T_oos : cr.data.T;
            sr.n_probs = spec->n_probs;
            memcpy(sr.probs, spec->probs, sizeof(sr.probs));
            const bool arg = (spec->argmax >> b) & 1u;
            sr.argmax_prob = arg ? spec->argmax_prob : -1.0;
            void *vals = *(void **)((char *)&cq + fo);
            if (i32)
                sr.values_i32 = (const int32_t *)vals;
            else
                sr.values_f64 = (const double *)vals;
            ls = launch_summary(&sr, (double *)((char *)dsum + pl.qoff[b]),
                                arg ? (int32_t *)((char *)dsum + pl.aoff[b]) : nullptr, st);
        }
        if (ls != HHMM_OK)
            break;
        size_t ho = pl.total;
        if ((e = hipMemcpyAsync(hout, dsum, pl.total, hipMemcpyDeviceToHost, st)) != hipSuccess)
            break;
        for (size_t j : pair_arrays) {
            if ((e = hipMemcpyAsync((char *)hout + ho, (char *)dslot + L.off[j], (size_t)L.P * 8,
                                    hipMemcpyDeviceToHost, st)) != hipSuccess)
                break;
            ho += (size_t)L.P * 8;
        }
        if (e != hipSuccess ||
            (e = hipMemcpyAsync((char *)hout + ho, (char *)dslot + L.status_off, (size_t)L.P * 4,
                                hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = sync_request(st)) != hipSuccess)
            break;
        move_summaries(c, pl, true);
        ho = pl.total;
        for (size_t j : pair_arrays) {
            memcpy((char *)arrays[j].host + (size_t)c.off[PAIRS] * 8, (char *)hout + ho, (size_t)L.P * 8);
            ho += (size_t)L.P * 8;
        }
        const int32_t *q = (const int32_t *)((char *)hout + ho);
        memcpy(status + c.off[PAIRS], q, (size_t)L.P * 4);
        fails += count_nonzero(q, L.P);
    }
    if (ls != HHMM_OK || e != hipSuccess) /* nothing of this request still runs when its buffers are pooled again */
        return fail_drained(ls, e, [&]() { return sync_request(st); }, cleanup,
                            "summary run (copy or kernel execution)", "stream");
    cleanup();
    *failures = fails;
    return HHMM_OK;
}

static hhmm_status run_summary(const hhmm_request *req, const hhmm_summary_spec *spec, hhmm_result *pairs,
                               const hhmm_result *full, hhmm_summary_result *out)
{
    const int64_t P = npairs(req), N = req->data.n_series;
    std::vector<int> devs;
    if (req->device == HHMM_DEVICE_SET) {
        devs = device_set();
    } else {
        int dev = req->device;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess)
            return hip_fail(hipGetLastError(), "hipGetDevice");
        devs.push_back(dev);
    }
    const size_t ns = (size_t)std::min<int64_t>(N, (int64_t)devs.size()); /* series ranges only, never draws */
    std::vector<int32_t> status((size_t)P, 0);
    std::vector<int64_t> fails(ns, 0);
    int cur = 0;
    (void)hipGetDevice(&cur);
    const hhmm_status s = run_per_device(devs, ns, ns > 1 ? "range" : nullptr, [&](size_t i) {
        return run_summary_on_device(req, spec, full, out, N * (int64_t)i / (int64_t)ns,
                                     N * (int64_t)(i + 1) / (int64_t)ns, ns > 1, status.data(), &fails[i]);
    });
    if (req->device == HHMM_DEVICE_SET)
        (void)hipSetDevice(cur);
    if (s != HHMM_OK)
        return s;
    return report_pairs(status, P, pairs ? pairs->pair_status : nullptr, fails);
}

template <class T> static void add_one(char *e, size_t n)
{
    for (size_t k = 0; k < n; ++k, e += sizeof(T)) {
        T v;
        memcpy(&v, e, sizeof(T));
        v += 1;
        memcpy(e, &v, sizeof(T));
    }
}

/* The host staging of hhmm_run without a device: every shard of `nshards`
 * cut into `nchunks` chunks, each chunk gathered into a heap slot (checked
 * byte for byte against a row-by-row pack of the same slices), "run" (every
 * output element + 1, every pair status 1) and scattered back -- through the
 * gather_chunk / scatter_chunk that run_on_device calls.  outputs_up: the
 * outputs are staged up whatever the request (else as hhmm_run does: when it
 * is ragged); status: where the pair statuses go (NULL: nowhere). */
static hhmm_status selftest_staging(const hhmm_request *req, hhmm_result *res, int nshards, int nchunks,
                                    bool outputs_up, int32_t *status)
{
    hhmm_request dreq = *req;
    hhmm_result dres = *res;
    std::vector<ArrayDesc> arrays;
    describe(req, res, &dreq, &dres, arrays);
    const bool ragged = outputs_up || req->data.T != nullptr || req->data.T_oos != nullptr;
    for (const Shard &sh : make_shards(req, nshards)) {
        for (const Shard &c : split_shard(req, sh, nchunks)) {
            const ChunkLayout L = chunk_layout(req, arrays, c, ragged);
            if (L.P < 1 || !chunk_pairs_agree(req, c, L)) { /* run_on_device's guard */
                set_error("pipeline self-test: a chunk stages %lld pairs for a sub-request of %lld",
                          (long long)chunk_staged_pairs(req, c), (long long)L.P);
                return HHMM_ERR_INVALID_ARGUMENT;
            }
            std::vector<char> slot(L.total, 0);
            gather_chunk(arrays, L, slot.data());
            for (size_t i = 0; i < arrays.size(); ++i) {
                const ArrayDesc &a = arrays[i];
                if (L.off[i] >= L.in_end)
                    continue;
                std::vector<char> ref(shard_bytes(a, L.sh));
                copy_shard_host(ref.data(), a.host, a, L.sh, true);
                if (memcmp(ref.data(), slot.data() + L.off[i], ref.size()) != 0) {
                    set_error("pipeline self-test: the staged slice of an input differs");
                    return HHMM_ERR_INVALID_ARGUMENT;
                }
            }
            for (size_t i = 0; i < arrays.size(); ++i) /* the "kernel" */
                if (arrays[i].output) {
                    const size_t n = shard_bytes(arrays[i], L.sh) / arrays[i].esize;
                    if (arrays[i].esize == sizeof(double))
                        add_one<double>(slot.data() + L.off[i], n);
                    else
                        add_one<int32_t>(slot.data() + L.off[i], n);
                }
            add_one<int32_t>(slot.data() + L.status_off, (size_t)L.P); /* the slot is zeroed: status 1 */
            const int64_t bad = scatter_chunk(arrays, L, slot.data() + L.out_begin, status, npairs(req));
            if (bad != L.P) {
                set_error("pipeline self-test: the scatter counted %lld failed pairs of %lld", (long long)bad,
                          (long long)L.P);
                return HHMM_ERR_INVALID_ARGUMENT;
            }
        }
    }
    return HHMM_OK;
}

} // namespace hhmm

using namespace hhmm;

extern "C" {

const char *hhmm_version(void) { return "hhmm-mi355x 0.3.0 gfx950 abi 2 src " HHMM_SOURCE_HASH; }

const char *hhmm_last_error(void) { return g_last_error.c_str(); }

int64_t hhmm_num_pairs(const hhmm_request *req) { return npairs(req); }

hhmm_status hhmm_validate(const hhmm_request *req, const hhmm_result *res, int host_pointers)
{
    return validate(req, res, host_pointers != 0);
}

hhmm_status hhmm_init(int ndev)
{
    hhmm_status s = check_device();
    if (s != HHMM_OK)
        return s;
    int n = 0;
    (void)hipGetDeviceCount(&n);
    if (ndev > n) {
        set_error("%d devices requested, %d visible", ndev, n);
        return HHMM_ERR_NO_DEVICE;
    }
    std::vector<int> d;
    for (int i = 0; i < (ndev > 0 ? ndev : 1); ++i) {
        if ((s = check_arch(i)) != HHMM_OK)
            return s;
        d.push_back(i);
    }
    std::lock_guard<std::mutex> g(devset().mu);
    devset().devs = d; /* HHMM_DEVICE_SET shards over devices 0 .. ndev-1 */
    return HHMM_OK;
}

hhmm_status hhmm_shutdown(void)
{
    pool_release_all();
    host_release_all();
    return HHMM_OK;
}

hhmm_status hhmm_workspace_size(const hhmm_request *req, size_t *bytes)
{
    if (!req || !bytes) {
        set_error("NULL argument");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const int64_t P = npairs(req);
    if (P < 1) {
        set_error("request describes no pairs");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    *bytes = workspace_bytes(req->model, req->data.K, req->data.L, req->data.T_max, req->data.T_oos_max, P, req->outputs,
                            (uint32_t)req->flags, req->data.n_series, req->pairing);
    return HHMM_OK;
}

hhmm_status hhmm_selftest_plan(const hhmm_request *req, char *buf, size_t n)
{
    if (!req || !buf || n == 0 || npairs(req) < 1) {
        set_error("NULL argument, or a request that describes no pairs");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return selftest_plan(req, npairs(req), buf, n);
}

hhmm_status hhmm_run_device(const hhmm_request *req, hhmm_result *res, void *workspace, size_t workspace_bytes_,
                            void *stream)
{
    hhmm_status s = validate(req, res, false);
    if (s != HHMM_OK)
        return s;
    if (!device_supported(req->model)) {
        set_error("model %d has no gfx950 path in this build", req->model);
        return HHMM_ERR_UNSUPPORTED;
    }
    if ((s = check_device()) != HHMM_OK)
        return s;
    size_t need = 0;
    hhmm_workspace_size(req, &need);
    if (workspace_bytes_ < need || (!workspace && need > 256)) {
        set_error("workspace of %zu bytes < %zu required", workspace_bytes_, need);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    /* the data arrays are device memory: their data-block bounds are checked on
     * the device, pair by pair (HHMM_PAIR_INVALID_DATA) */
    return launch_all(req, res, npairs(req), workspace, (hipStream_t)stream, nullptr, 0, true);
}

hhmm_status hhmm_run(const hhmm_request *req, hhmm_result *res)
{
    hhmm_status s = validate(req, res, true);
    if (s != HHMM_OK)
        return s;
    if (!device_supported(req->model)) {
        set_error("model %d has no gfx950 path in this build", req->model);
        return HHMM_ERR_UNSUPPORTED;
    }
    if ((s = check_device()) != HHMM_OK)
        return s;
    if (req->device == HHMM_DEVICE_SET)
        return run_sharded(req, res);
    int dev = req->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess)
            return hip_fail(hipGetLastError(), "hipGetDevice");
    }
    hipError_t e = hipSetDevice(dev);
    if (e != hipSuccess)
        return hip_fail(e, "hipSetDevice");
    const int64_t P = npairs(req);
    std::vector<int32_t> status((size_t)P, 0);
    std::vector<int64_t> fails(1, 0);
    s = run_on_device(req, res, whole_shard(req), status.data(), &fails[0]);
    if (s != HHMM_OK)
        return s;
    return report_pairs(status, P, res->pair_status, fails);
}

hhmm_status hhmm_run_summary(const hhmm_request *req, const hhmm_summary_spec *spec, hhmm_result *pairs,
                             hhmm_summary_result *out)
{
    REQUIRE(req && spec && pairs && out, "request, spec, pairs and out must be non-NULL");
    REQUIRE(req->pairing != HHMM_PAIR_ZIP, "hhmm_run_summary: ZIP pairing has one draw per series, nothing to reduce");
    REQUIRE(spec->n_probs >= 1 && spec->n_probs <= HHMM_SUMMARY_MAX_PROBS, "summary needs 1 <= n_probs <= %d (got %d)",
            HHMM_SUMMARY_MAX_PROBS, spec->n_probs);
    for (int j = 0; j < spec->n_probs; ++j)
        REQUIRE(spec->probs[j] >= 0.0 && spec->probs[j] <= 1.0, "summary probs[%d] = %g outside [0, 1]", j,
                spec->probs[j]);
    REQUIRE((spec->summarise & ~kSumStepBits) == 0, "summarise 0x%x holds bits that are no per-step output",
            spec->summarise & ~kSumStepBits);
    REQUIRE((req->outputs & kSumStepBits & ~spec->summarise) == 0,
            "per-step outputs 0x%x are requested but not in spec->summarise (hhmm_run_summary returns no per-draw "
            "array; use hhmm_run)", req->outputs & kSumStepBits & ~spec->summarise);
    REQUIRE((spec->argmax & ~(spec->summarise & kSumKAxisBits)) == 0,
            "argmax 0x%x must be a subset of summarise with a K axis", spec->argmax);
    if (spec->argmax)
        REQUIRE(spec->argmax_prob >= 0.0 && spec->argmax_prob <= 1.0, "summary argmax_prob = %g outside [0, 1]",
                spec->argmax_prob);
    for (int b = 0; b < 32; ++b) {
        if ((spec->summarise >> b) & 1u)
            REQUIRE(out->quantiles[b], "summary of output bit %d requested but out->quantiles[%d] is NULL", b, b);
        if ((spec->argmax >> b) & 1u)
            REQUIRE(out->argmax[b], "argmax of output bit %d requested but out->argmax[%d] is NULL", b, b);
    }
    hhmm_request r2 = *req;
    r2.outputs |= spec->summarise;
    /* what validate() and describe() see: the caller's [P] pointers, and for the
     * per-step outputs (device-only here) a placeholder that is never dereferenced */
    hhmm_result full{};
    full.loglik = pairs->loglik;
    full.logp_zstar = pairs->logp_zstar;
    full.pair_status = pairs->pair_status;
    static double placeholder;
    for (int b = 0; b < 32; ++b) {
        bool i32 = false;
        const size_t fo = sum_field(b, i32);
        if (((spec->summarise >> b) & 1u) && fo != (size_t)-1)
            *(void **)((char *)&full + fo) = &placeholder;
    }
    hhmm_status s = validate(&r2, &full, true);
    if (s != HHMM_OK)
        return s;
    const int64_t P = npairs(&r2), N = r2.data.n_series;
    if (P / N > HHMM_SUMMARY_MAX_DRAWS) {
        set_error("summary of S = %lld draws per series: at most %d (one cell is sorted in one workgroup's LDS)",
                  (long long)(P / N), HHMM_SUMMARY_MAX_DRAWS);
        return HHMM_ERR_UNSUPPORTED;
    }
    if (!device_supported(r2.model)) {
        set_error("model %d has no gfx950 path in this build", r2.model);
        return HHMM_ERR_UNSUPPORTED;
    }
    if ((s = check_device()) != HHMM_OK)
        return s;
    return run_summary(&r2, spec, pairs, &full, out);
}

int hhmm_device_set(int32_t *ordinals, int capacity)
{
    const std::vector<int> d = device_set();
    for (int i = 0; i < (int)d.size() && i < capacity; ++i)
        if (ordinals)
            ordinals[i] = d[(size_t)i];
    return (int)d.size();
}

hhmm_status hhmm_init_devices(const int32_t *ordinals, int n)
{
    hhmm_status s = check_device();
    if (s != HHMM_OK)
        return s;
    if (!ordinals || n < 1) {
        set_error("hhmm_init_devices needs n >= 1 ordinals");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    int vis = 0;
    (void)hipGetDeviceCount(&vis);
    std::vector<int> d;
    for (int i = 0; i < n; ++i) {
        if (ordinals[i] < 0 || ordinals[i] >= vis) {
            set_error("device ordinal %d not visible (%d devices)", ordinals[i], vis);
            return HHMM_ERR_NO_DEVICE;
        }
        if ((s = check_arch(ordinals[i])) != HHMM_OK)
            return s;
        d.push_back(ordinals[i]);
    }
    std::lock_guard<std::mutex> g(devset().mu);
    devset().devs = d;
    return HHMM_OK;
}

/* ---- one series split over ranks along T (include/hhmm.h hhmm_segment) ---- */
static hhmm_status segment_check(const hhmm_request *req, const hhmm_segment *seg, hhmm_request &r2)
{
    if (!req || !seg) {
        set_error("NULL argument");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const int m = req->model;
    if (!hmm_has_backward(m) || req->data.K > kMaxKLarge ||
        (req->data.K > kMaxK && m != HHMM_MODEL_HMM_MULTINOM && m != HHMM_MODEL_HMM_GAUSS)) {
        set_error("segment windows: the HMM family at K <= %d (hmm, hmm-multinom, semisup, tayal), "
                  "hmm and hmm-multinom at K <= %d", kMaxK, kMaxKLarge);
        return HHMM_ERR_UNSUPPORTED;
    }
    const uint32_t ok = kOutFb & ~kOutLog;
    if (req->outputs & ~ok) {
        set_error("segment windows: outputs 0x%x have no segment form (loglik, alpha_tk, beta_tk, ungamma_tk, "
                  "gamma_tk only; the Viterbi and FFBS stay sequential per pair)", req->outputs & ~ok);
        return HHMM_ERR_UNSUPPORTED;
    }
    if (req->data.T) {
        set_error("segment windows: every series spans the whole window (data.T must be NULL)");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (req->abi_version != HHMM_ABI_VERSION || npairs(req) < 1 || req->data.T_max < 1 || req->data.K < 1 ||
        (is_discrete(m) && (req->data.L < 1 || !req->data.x_int)) || (m == HHMM_MODEL_HMM_GAUSS && !req->data.x_real)) {
        set_error("segment windows: malformed request (abi, pairs, T_max, K, L or observations)");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    r2 = *req;
    r2.flags = (req->flags & ~(int32_t)HHMM_FLAG_SCAN_OFF) | (int32_t)HHMM_FLAG_SCAN_FORCE;
    return HHMM_OK;
}

hhmm_status hhmm_segment_workspace_size(const hhmm_request *req, size_t *bytes)
{
    hhmm_segment dummy{1, 1, nullptr, nullptr, nullptr};
    hhmm_request r2;
    hhmm_status s = segment_check(req, &dummy, r2);
    if (s != HHMM_OK)
        return s;
    return hhmm_workspace_size(&r2, bytes);
}

static hhmm_status segment_run(const hhmm_request *req, hhmm_result *res, const hhmm_segment *seg, void *ws,
                               size_t wsb, void *stream, int phase)
{
    hhmm_request r2;
    hhmm_status s = segment_check(req, seg, r2);
    if (s != HHMM_OK)
        return s;
    hhmm_result empty;
    memset(&empty, 0, sizeof(empty));
    hhmm_result *rr = res ? res : &empty;
    if (phase == 1) {
        if (!seg->summary) {
            set_error("segment summary: seg->summary is NULL");
            return HHMM_ERR_INVALID_ARGUMENT;
        }
        /* the request side (draw and data pointers) before any launch */
        if ((s = validate_impl(&r2, nullptr, false)) != HHMM_OK)
            return s;
    } else {
        if ((!seg->first && !seg->enter) || (!seg->last && !seg->leave)) {
            set_error("segment finish: a window that is not first needs enter, one that is not last needs leave");
            return HHMM_ERR_INVALID_ARGUMENT;
        }
        if ((s = validate(&r2, rr, false)) != HHMM_OK)
            return s;
    }
    if ((s = check_device()) != HHMM_OK)
        return s;
    size_t need = 0;
    hhmm_workspace_size(&r2, &need);
    if (wsb < need || !ws) {
        set_error("workspace of %zu bytes < %zu required (hhmm_segment_workspace_size)", wsb, need);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    /* both calls check the window's data: the summary marks a bad pair's record
     * (a log scale of +infinity) so that every rank chaining it flags the pair */
    return launch_all(&r2, rr, npairs(&r2), ws, (hipStream_t)stream, seg, phase, true);
}

hhmm_status hhmm_segment_summary_device(const hhmm_request *req, const hhmm_segment *seg, void *workspace,
                                        size_t workspace_bytes_, void *stream)
{
    return segment_run(req, nullptr, seg, workspace, workspace_bytes_, stream, 1);
}

hhmm_status hhmm_segment_finish_device(const hhmm_request *req, hhmm_result *res, const hhmm_segment *seg,
                                       void *workspace, size_t workspace_bytes_, void *stream)
{
    return segment_run(req, res, seg, workspace, workspace_bytes_, stream, 2);
}

hhmm_status hhmm_selftest_shards(const hhmm_request *req, hhmm_result *res, int nshards)
{
    hhmm_status s = validate(req, res, true);
    if (s != HHMM_OK)
        return s;
    if (nshards < 1) {
        set_error("nshards must be >= 1");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return selftest_staging(req, res, nshards, 1, true, nullptr);
}

hhmm_status hhmm_selftest_pipeline(const hhmm_request *req, hhmm_result *res, int nshards, int nchunks)
{
    hhmm_status s = validate(req, res, true);
    if (s != HHMM_OK)
        return s;
    if (nshards < 1 || nchunks < 1) {
        set_error("nshards and nchunks must be >= 1");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return selftest_staging(req, res, nshards, nchunks, false, res->pair_status);
}

hhmm_status hhmm_selftest_cr_log(const double *in, double *out, int64_t n)
{
    hhmm_status s = check_device();
    if (s != HHMM_OK)
        return s;
    return selftest_cr_math(in, out, n, 0);
}

hhmm_status hhmm_selftest_cr_exp(const double *in, double *out, int64_t n)
{
    hhmm_status s = check_device();
    if (s != HHMM_OK)
        return s;
    return selftest_cr_math(in, out, n, 1);
}

hhmm_status hhmm_selftest_det_log(const double *in, double *out, int64_t n)
{
    hhmm_status s = check_device();
    if (s != HHMM_OK)
        return s;
    return selftest_cr_math(in, out, n, 2);
}

hhmm_status hhmm_selftest_det_exp(const double *in, double *out, int64_t n)
{
    hhmm_status s = check_device();
    if (s != HHMM_OK)
        return s;
    return selftest_cr_math(in, out, n, 3);
}

} /* extern "C" */

/* ------------------------------------------------------------------ */
/* Feature extractor entry points (include/hhmm_features.h)            */
/* ------------------------------------------------------------------ */

extern "C" {

static hhmm_status check_ticks(const hhmm_ticks *tk, const hhmm_legs *lg)
{
    if (!tk || !lg) {
        set_error("NULL ticks / legs");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (tk->n < 3 || tk->n > 0x7fffffffLL) {
        set_error("n = %lld ticks outside 3..2^31-1", (long long)tk->n);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (!tk->price || !tk->size || !tk->time) {
        set_error("price, size and time are required");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (lg->capacity < 0) {
        set_error("negative leg capacity");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return HHMM_OK;
}

hhmm_status hhmm_features_workspace_size(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0) {
        set_error("bad argument");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    *bytes = features_workspace_bytes(n);
    return HHMM_OK;
}

hhmm_status hhmm_extract_features_device(const hhmm_ticks *ticks, hhmm_legs *legs, void *workspace,
                                         size_t workspace_bytes_, void *stream)
{
    hhmm_status s = check_ticks(ticks, legs);
    if (s != HHMM_OK)
        return s;
    if ((s = check_device()) != HHMM_OK)
        return s;
    return features_run_device(ticks, legs, workspace, workspace_bytes_, (hipStream_t)stream);
}

hhmm_status hhmm_extract_features(const hhmm_ticks *ticks, hhmm_legs *legs, int device)
{
    hhmm_status s = check_ticks(ticks, legs);
    if (s != HHMM_OK)
        return s;
    if ((s = check_device()) != HHMM_OK)
        return s;
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess)
        return hip_fail(hipGetLastError(), "hipGetDevice");
    hipError_t e = hipSetDevice(dev);
    if (e != hipSuccess)
        return hip_fail(e, "hipSetDevice");
    const int64_t n = ticks->n;
    const int64_t cap = legs->capacity;
    std::vector<void *> owned;
    auto cleanup = [&]() {
        for (void *p : owned)
            pool_put(p);
    };
    auto get = [&](size_t bytes) -> void * {
        void *p = pool_get(dev, bytes ? bytes : 8);
        if (p)
            owned.push_back(p);
        return p;
    };
    hhmm_ticks dt = *ticks;
    const double *hin[3] = {ticks->price, ticks->size, ticks->time};
    const double **din[3] = {&dt.price, &dt.size, &dt.time};
    for (int i = 0; i < 3; ++i) {
        void *p = get(sizeof(double) * (size_t)n);
        if (!p) {
            cleanup();
            set_error("device allocation failed (ticks)");
            return HHMM_ERR_OUT_OF_MEMORY;
        }
        e = hipMemcpy(p, hin[i], sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            cleanup();
            return hip_fail(e, "hipMemcpy H2D (ticks)");
        }
        *din[i] = (const double *)p;
    }
    hhmm_legs dl = *legs;
    struct Col {
        void *host;
        void **dev;
        size_t es;
    } cols[] = {{legs->price, (void **)&dl.price, 8},     {legs->start, (void **)&dl.start, 4},
                {legs->end, (void **)&dl.end, 4},         {legs->size_av, (void **)&dl.size_av, 8},
                {legs->f0, (void **)&dl.f0, 4},           {legs->f1, (void **)&dl.f1, 4},
                {legs->f2, (void **)&dl.f2, 4},           {legs->feature, (void **)&dl.feature, 4},
                {legs->trend, (void **)&dl.trend, 4},     {legs->x, (void **)&dl.x, 4},
                {legs->sign, (void **)&dl.sign, 4}};
    for (auto &c : cols) {
        if (!c.host || cap == 0) {
            *c.dev = nullptr;
            continue;
        }
        void *p = get(c.es * (size_t)cap);
        if (!p) {
            cleanup();
            set_error("device allocation failed (legs)");
            return HHMM_ERR_OUT_OF_MEMORY;
        }
        *c.dev = p;
    }
    const size_t wsb = features_workspace_bytes(n);
    void *ws = get(wsb);
    if (!ws) {
        cleanup();
        set_error("workspace allocation of %zu bytes failed", wsb);
        return HHMM_ERR_OUT_OF_MEMORY;
    }
    s = features_run_device(&dt, &dl, ws, wsb, nullptr);
    legs->n_legs = dl.n_legs;
    if (s == HHMM_OK) {
        for (auto &c : cols) {
            if (!*c.dev)
                continue;
            e = hipMemcpy(c.host, *c.dev, c.es * (size_t)dl.n_legs, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                cleanup();
                return hip_fail(e, "hipMemcpy D2H (legs)");
            }
        }
    }
    cleanup();
    return s;
}

} // extern "C"
