/*
 * hhmm_stage.cpp -- the plan and the host staging of a host-array request
 * (hhmm_stage.h): no HIP, no kernels' launch plan.
 */
#include "hhmm_stage.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <emmintrin.h>

namespace hhmm {

int64_t npairs(const hhmm_request *r)
{
    if (!r)
        return -1;
    if (r->data.n_series < 1 || r->draws.n_draws < 1)
        return -1;
    if (r->pairing == HHMM_PAIR_ZIP)
        return r->data.n_series == r->draws.n_draws ? r->data.n_series : -1;
    if (r->pairing == HHMM_PAIR_GRID)
        return r->data.n_series * r->draws.n_draws;
    if (r->pairing == HHMM_PAIR_BLOCK)
        return r->draws.n_draws % r->data.n_series == 0 ? r->draws.n_draws : -1;
    return -1;
}

/* The pointer field at byte `off` of a request / result. */
static const void *get_field(const void *base, size_t off)
{
    const void *p;
    memcpy(&p, (const char *)base + off, sizeof(p));
    return p;
}
static void set_field(void *base, size_t off, const void *p)
{
    memcpy((char *)base + off, &p, sizeof(p));
}

void describe(const hhmm_request *r, const hhmm_result *o, hhmm_request *dr, hhmm_result *dq,
              std::vector<ArrayDesc> &v)
{
    const hhmm_data &d = r->data;
    const hhmm_draws &w = r->draws;
    const size_t N = (size_t)d.n_series, S = (size_t)w.n_draws, Tm = (size_t)d.T_max;
    const size_t To = (size_t)(d.T_oos_max > 0 ? d.T_oos_max : 0);
    const size_t K = (size_t)d.K, L = (size_t)(d.L > 0 ? d.L : 0), M = (size_t)(d.M > 0 ? d.M : 0);
    const size_t P = (size_t)npairs(r);
    auto in = [&](size_t field, size_t n, size_t es, int cls) {
        if (const void *h = get_field(r, field))
            v.push_back({h, false, field, n, es, false, cls});
    };
    auto ou = [&](uint32_t bit, size_t field, size_t n, size_t es) {
        const void *h = get_field(o, field);
        if ((r->outputs & bit) && h)
            v.push_back({h, true, field, n, es, true, PAIRS});
        else
            set_field(dq, field, nullptr);
    };
    in(offsetof(hhmm_request, data.T), N, 4, SERIES);
    in(offsetof(hhmm_request, data.x_int), N * Tm, 4, SERIES);
    in(offsetof(hhmm_request, data.x_real), N * Tm, 8, SERIES);
    in(offsetof(hhmm_request, data.g), N * Tm, 4, SERIES);
    in(offsetof(hhmm_request, data.sign), N * Tm, 4, SERIES);
    in(offsetof(hhmm_request, data.u), N * Tm * M, 8, SERIES);
    in(offsetof(hhmm_request, data.T_oos), N, 4, SERIES);
    in(offsetof(hhmm_request, data.x_oos), N * To, 4, SERIES);
    in(offsetof(hhmm_request, data.sign_oos), N * To, 4, SERIES);
    dr->data.hyperparams = nullptr;
    in(offsetof(hhmm_request, draws.p_1k), S * K, 8, DRAWS);
    in(offsetof(hhmm_request, draws.A_ij), S * K * K, 8, DRAWS);
    in(offsetof(hhmm_request, draws.phi_k), S * K * L, 8, DRAWS);
    in(offsetof(hhmm_request, draws.mu_k), S * K, 8, DRAWS);
    in(offsetof(hhmm_request, draws.sigma_k), S * K, 8, DRAWS);
    in(offsetof(hhmm_request, draws.w_km), S * K * M, 8, DRAWS);
    in(offsetof(hhmm_request, draws.b_km), S * K * M, 8, DRAWS);
    in(offsetof(hhmm_request, draws.s_k), S * K, 8, DRAWS);
    in(offsetof(hhmm_request, draws.lambda_kl), S * K * L, 8, DRAWS);
    in(offsetof(hhmm_request, draws.mu_kl), S * K * L, 8, DRAWS);
    in(offsetof(hhmm_request, draws.s_kl), S * K * L, 8, DRAWS);
    in(offsetof(hhmm_request, draws.p_11), S, 8, DRAWS);
    in(offsetof(hhmm_request, draws.A_row), S * 4, 8, DRAWS);
    in(offsetof(hhmm_request, ffbs_u), P * Tm, 8, PAIRS);
    in(offsetof(hhmm_request, hat_rand), P * Tm * 3, 8, PAIRS);
    const size_t Tz = (r->model == HHMM_MODEL_TAYAL_LITE) ? To : Tm;
    ou(HHMM_OUT_LOGLIK, offsetof(hhmm_result, loglik), P, 8);
    ou(HHMM_OUT_UNALPHA, offsetof(hhmm_result, unalpha_tk), P * Tm * K, 8);
    ou(HHMM_OUT_ALPHA, offsetof(hhmm_result, alpha_tk), P * Tm * K, 8);
    ou(HHMM_OUT_UNBETA, offsetof(hhmm_result, unbeta_tk), P * Tm * K, 8);
    ou(HHMM_OUT_BETA, offsetof(hhmm_result, beta_tk), P * Tm * K, 8);
    ou(HHMM_OUT_UNGAMMA, offsetof(hhmm_result, ungamma_tk), P * Tm * K, 8);
    ou(HHMM_OUT_GAMMA, offsetof(hhmm_result, gamma_tk), P * Tm * K, 8);
    ou(HHMM_OUT_ZSTAR, offsetof(hhmm_result, zstar_t), P * Tz, 4);
    ou(HHMM_OUT_LOGP_ZSTAR, offsetof(hhmm_result, logp_zstar), P, 8);
    ou(HHMM_OUT_OBLIK_TK, offsetof(hhmm_result, oblik_tk), P * Tm * K, 8);
    ou(HHMM_OUT_OBLIK_T, offsetof(hhmm_result, oblik_t), P * Tm, 8);
    ou(HHMM_OUT_FFBS, offsetof(hhmm_result, z_ffbs), P * Tm, 4);
    ou(HHMM_OUT_ALPHA_OOS, offsetof(hhmm_result, alpha_tk_oos), P * To * K, 8);
    ou(HHMM_OUT_UNALPHA_OOS, offsetof(hhmm_result, unalpha_tk_oos), P * To * K, 8);
    ou(HHMM_OUT_LOGA, offsetof(hhmm_result, logA_ij), P * Tm * K, 8);
    ou(HHMM_OUT_HATPI, offsetof(hhmm_result, hatpi_tk), P * Tm * K, 8);
    ou(HHMM_OUT_HATZ, offsetof(hhmm_result, hatz_t), P * Tm, 4);
    ou(HHMM_OUT_HATL, offsetof(hhmm_result, hatl_t), P * Tm, 4);
    ou(HHMM_OUT_HATX, offsetof(hhmm_result, hatx_t), P * Tm, 8);
}

Shard whole_shard(const hhmm_request *r)
{
    const int64_t N = r->data.n_series, S = r->draws.n_draws, P = npairs(r);
    return Shard{{0, 0, 0}, {N, S, P}, {N, S, P}};
}

/* `n` contiguous ranges of the series [a0, a1) with all their draws (GRID:
 * every draw; ZIP / BLOCK: the series' own) -- never a split by draws. */
std::vector<Shard> series_ranges(const hhmm_request *r, int64_t a0, int64_t a1, int64_t n)
{
    const int64_t N = r->data.n_series, S = r->draws.n_draws, P = npairs(r);
    const int64_t B = S / N; /* ZIP: 1 */
    n = std::max<int64_t>(1, std::min(n, a1 - a0));
    std::vector<Shard> v;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = a0 + (a1 - a0) * i / n, b = a0 + (a1 - a0) * (i + 1) / n;
        if (r->pairing != HHMM_PAIR_GRID)
            v.push_back(Shard{{a, B * a, B * a}, {b - a, B * (b - a), B * (b - a)}, {N, S, P}});
        else
            v.push_back(Shard{{a, 0, S * a}, {b - a, S, S * (b - a)}, {N, S, P}});
    }
    return v;
}

/* Splits a request over `n` shards: contiguous series ranges; a GRID request
 * with fewer series than shards splits its draws instead (pairs p = s + S*n
 * with s in the range: rows of S' pairs at a pitch of S). */
std::vector<Shard> make_shards(const hhmm_request *r, int n)
{
    const int64_t N = r->data.n_series, S = r->draws.n_draws;
    if (r->pairing != HHMM_PAIR_GRID || N >= n)
        return series_ranges(r, 0, N, n);
    const int64_t ns = std::min<int64_t>(n, S);
    std::vector<Shard> v;
    for (int64_t i = 0; i < ns; ++i) {
        const int64_t a = S * i / ns, b = S * (i + 1) / ns;
        v.push_back(Shard{{0, a, a}, {N, b - a, b - a}, {N, S, S}});
    }
    return v;
}

/* Sub-shards of a device shard: `n` contiguous ranges of its units (series,
 * or draws for a GRID request split by draws), each a Shard of the request. */
std::vector<Shard> split_shard(const hhmm_request *r, const Shard &sh, int64_t n)
{
    const int64_t S = r->draws.n_draws;
    if (n <= 1)
        return {sh};
    /* a GRID shard holding every series splits by draws (rows of the chunk's
     * draws at a pitch of S pairs) when it is a draws shard already or has
     * fewer series than chunks; every other shard splits by series.  A draws
     * shard is known by its layout (its pairs lie at a pitch of S, not packed
     * over the request's P), not by holding fewer than S draws: at S = 1 it
     * holds them all.  With one series the two layouts coincide and the shard
     * splits by draws through `cnt[SERIES] < n`. */
    const bool all_series = sh.cnt[SERIES] == r->data.n_series;
    const bool draws_shard = sh.lead[PAIRS] != npairs(r);
    const bool by_draws = r->pairing == HHMM_PAIR_GRID && all_series && (draws_shard || sh.cnt[SERIES] < n);
    const int64_t u0 = by_draws ? sh.off[DRAWS] : sh.off[SERIES];
    const int64_t units = by_draws ? sh.cnt[DRAWS] : sh.cnt[SERIES];
    const int64_t ns = std::max<int64_t>(1, std::min(n, units));
    std::vector<Shard> v;
    for (int64_t i = 0; i < ns; ++i) {
        const int64_t a = u0 + units * i / ns, b = u0 + units * (i + 1) / ns;
        Shard c = sh;
        if (by_draws) {
            c.lead[PAIRS] = S;
            c.off[DRAWS] = c.off[PAIRS] = a;
            c.cnt[DRAWS] = c.cnt[PAIRS] = b - a;
        } else {
            const int64_t per = sh.cnt[SERIES] > 0 ? sh.cnt[PAIRS] / sh.cnt[SERIES] : 0; /* pairs per series */
            const int64_t dper = sh.cnt[SERIES] > 0 ? sh.cnt[DRAWS] / sh.cnt[SERIES] : 0;
            c.off[SERIES] = a;
            c.cnt[SERIES] = b - a;
            c.off[PAIRS] = sh.off[PAIRS] + (a - u0) * per;
            c.cnt[PAIRS] = (b - a) * per;
            if (r->pairing != HHMM_PAIR_GRID) { /* ZIP / BLOCK: the series' own draws */
                c.off[DRAWS] = sh.off[DRAWS] + (a - u0) * dper;
                c.cnt[DRAWS] = (b - a) * dper;
            }
        }
        v.push_back(c);
    }
    return v;
}

ShardRows shard_rows(const void *host, const ArrayDesc &a, const Shard &sh)
{
    const size_t es = a.esize, lead = (size_t)sh.lead[a.cls], cnt = (size_t)sh.cnt[a.cls];
    return ShardRows{(char *)host + (size_t)sh.off[a.cls] * es, a.elems / lead, cnt * es, lead * es};
}

void copy_shard_host(void *packed, const void *host, const ArrayDesc &a, const Shard &sh, bool to_packed)
{
    const ShardRows r = shard_rows(host, a, sh);
    for (size_t i = 0; i < r.rows; ++i) {
        char *h = r.base + i * r.pitch, *q = (char *)packed + i * r.width;
        if (to_packed)
            memcpy(q, h, r.width);
        else
            memcpy(h, q, r.width);
    }
}

void run_parallel(size_t n, const std::function<void(size_t)> &fn)
{
    if (n == 0)
        return;
    std::vector<std::thread> th;
    std::vector<size_t> mine{0};
    for (size_t i = 1; i < n; ++i) {
        try {
            th.emplace_back([&fn, i] { fn(i); });
        } catch (...) {
            mine.push_back(i);
        }
    }
    for (size_t i : mine)
        fn(i);
    for (auto &t : th)
        t.join();
}

/* One row of a staging copy.  Large rows leave the cache alone: the
 * destination is written with streaming stores (no read-for-ownership of the
 * caller's lines, which would double the DRAM traffic of the scatter into R's
 * arrays), 16 bytes at a time once it is 16-byte aligned. */
void copy_row(char *dst, const char *src, size_t n)
{
    if (n < 4096) {
        memcpy(dst, src, n);
        return;
    }
    const size_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    memcpy(dst, src, head);
    dst += head;
    src += head;
    n -= head;
    const size_t m = n & ~(size_t)63;
    for (size_t i = 0; i < m; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i *)(src + i));
        const __m128i b = _mm_loadu_si128((const __m128i *)(src + i + 16));
        const __m128i c = _mm_loadu_si128((const __m128i *)(src + i + 32));
        const __m128i d = _mm_loadu_si128((const __m128i *)(src + i + 48));
        _mm_stream_si128((__m128i *)(dst + i), a);
        _mm_stream_si128((__m128i *)(dst + i + 16), b);
        _mm_stream_si128((__m128i *)(dst + i + 32), c);
        _mm_stream_si128((__m128i *)(dst + i + 48), d);
    }
    memcpy(dst + m, src + m, n - m);
}

/* rows x width bytes between pitched buffers, split over host threads when
 * the copy is large (the staging copies run beside the GPU's DMA; up to 16
 * threads, the CPU share of one GPU on an 8-GPU node) */
void par_copy_rows(char *dst, size_t dpitch, const char *src, size_t spitch, size_t width, size_t rows)
{
    if (rows == 0 || width == 0)
        return;
    if (dpitch == width && spitch == width) { /* contiguous: one long row, split in pieces */
        width *= rows;
        rows = 1;
        dpitch = spitch = width;
    }
    const size_t total = width * rows;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nt = total < ((size_t)4 << 20) ? 1 : std::min<size_t>(16u, hw);
    /* work item i: a range of rows, or of bytes of the single row */
    run_parallel(nt, [&](size_t i) {
        if (rows >= nt) {
            const size_t r0 = rows * i / nt, r1 = rows * (i + 1) / nt;
            for (size_t r = r0; r < r1; ++r)
                copy_row(dst + r * dpitch, src + r * spitch, width);
        } else {
            for (size_t r = 0; r < rows; ++r) {
                const size_t b0 = (width * i / nt) & ~(size_t)63, b1 = i + 1 == nt ? width : (width * (i + 1) / nt) & ~(size_t)63;
                copy_row(dst + r * dpitch + b0, src + r * spitch + b0, b1 - b0);
            }
        }
        _mm_sfence(); /* this thread's streaming stores, before the join */
    });
}

size_t shard_bytes(const ArrayDesc &a, const Shard &sh)
{
    return a.elems / (size_t)sh.lead[a.cls] * (size_t)sh.cnt[a.cls] * a.esize;
}

ChunkLayout chunk_layout(const hhmm_request *req, const std::vector<ArrayDesc> &arrays, const Shard &sh, bool ragged)
{
    ChunkLayout L;
    L.sh = sh;
    hhmm_request r = *req;
    r.data.n_series = sh.cnt[SERIES];
    r.draws.n_draws = sh.cnt[DRAWS];
    L.P = npairs(&r);
    L.off.assign(arrays.size(), 0);
    size_t o = 0;
    auto place = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    };
    for (size_t i = 0; i < arrays.size(); ++i) /* inputs first */
        if (!arrays[i].output)
            L.off[i] = place(shard_bytes(arrays[i], sh));
    const size_t outs = o;
    for (size_t i = 0; i < arrays.size(); ++i)
        if (arrays[i].output)
            L.off[i] = place(shard_bytes(arrays[i], sh));
    L.status_off = place((size_t)L.P * sizeof(int32_t));
    L.total = o;
    /* outputs travel up too where padded steps must round-trip untouched */
    L.in_end = ragged ? L.status_off : outs;
    L.out_begin = outs;
    return L;
}

/* The pairs a chunk's PAIRS-class slices hold (rows of cnt at a pitch of lead)
 * must be the pairs its sub-request computes: the kernels write L.P pairs of
 * every output into slots sized from the slices, so a planner mistake here
 * would be a device overrun. */
int64_t chunk_staged_pairs(const hhmm_request *req, const Shard &c)
{
    return c.lead[PAIRS] > 0 ? c.cnt[PAIRS] * (npairs(req) / c.lead[PAIRS]) : -1;
}
bool chunk_pairs_agree(const hhmm_request *req, const Shard &c, const ChunkLayout &L)
{
    return chunk_staged_pairs(req, c) == L.P;
}

void gather_chunk(const std::vector<ArrayDesc> &arrays, const ChunkLayout &L, void *dst)
{
    for (size_t i = 0; i < arrays.size(); ++i) {
        const ArrayDesc &a = arrays[i];
        if (L.off[i] >= L.in_end)
            continue;
        const ShardRows r = shard_rows(a.host, a, L.sh);
        par_copy_rows((char *)dst + L.off[i], r.width, r.base, r.pitch, r.width, r.rows);
    }
}

int64_t count_nonzero(const int32_t *q, int64_t n)
{
    int64_t c = 0;
    for (int64_t p = 0; p < n; ++p)
        c += q[p] != 0;
    return c;
}

int64_t scatter_chunk(const std::vector<ArrayDesc> &arrays, const ChunkLayout &L, const void *src, int32_t *status,
                      int64_t P_request)
{
    for (size_t i = 0; i < arrays.size(); ++i) {
        const ArrayDesc &a = arrays[i];
        if (!a.output)
            continue;
        const ShardRows r = shard_rows(a.host, a, L.sh);
        par_copy_rows(r.base, r.pitch, (const char *)src + (L.off[i] - L.out_begin), r.width, r.width, r.rows);
    }
    const char *q = (const char *)src + (L.status_off - L.out_begin);
    if (status) { /* [P] in the caller's layout (a PAIRS array of P elements) */
        const ArrayDesc sa{status, true, offsetof(hhmm_result, pair_status), (size_t)P_request, sizeof(int32_t), true,
                           PAIRS};
        const ShardRows r = shard_rows(status, sa, L.sh);
        par_copy_rows(r.base, r.pitch, q, r.width, r.width, r.rows);
    }
    return count_nonzero((const int32_t *)q, L.P);
}

void bind_chunk(const std::vector<ArrayDesc> &arrays, const ChunkLayout &L, void *slot_base, const hhmm_request &dreq,
                const hhmm_result &dres, hhmm_request &cr, hhmm_result &cq)
{
    cr = dreq;
    cq = dres;
    cr.data.n_series = L.sh.cnt[SERIES];
    cr.draws.n_draws = L.sh.cnt[DRAWS];
    for (size_t i = 0; i < arrays.size(); ++i) {
        const ArrayDesc &a = arrays[i];
        set_field(a.in_result ? (void *)&cq : (void *)&cr, a.field, (char *)slot_base + L.off[i]);
    }
    cq.pair_status = (int32_t *)((char *)slot_base + L.status_off);
}

} // namespace hhmm
