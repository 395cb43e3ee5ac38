/*
 * hhmm_stage.h -- the plan and the host staging of a host-array request
 * (hhmm_run, hhmm_run_summary): which arrays a request has, how it splits
 * into shards and chunks, where a chunk's arrays sit in a staging slot, and
 * the pitched copies between the caller's arrays and a slot.  No HIP here: a
 * host compiler builds hhmm_stage.cpp on its own; what needs the kernels'
 * launch plan or a device stays in hhmm_api.cpp.  Not part of the public ABI.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "hhmm.h"

namespace hhmm {

/* Pairs of a request; -1 when its pairing and counts do not fit. */
int64_t npairs(const hhmm_request *r);

/* One array of the request: where it lives and how many elements. */
enum ArrayClass { SERIES = 0, DRAWS = 1, PAIRS = 2 }; /* leading (fastest) dimension N, S or P */
struct ArrayDesc {
    const void *host;
    bool in_result; /* its pointer is a field of hhmm_result (else of hhmm_request) ... */
    size_t field;   /* ... at this byte offset */
    size_t elems;
    size_t esize;
    bool output;
    int cls;        /* ArrayClass */
};

/* Every input / output array the request uses, inputs first.  *dr and *dq
 * (copies of *r and *o) lose what never travels: hyperparams and the outputs
 * that are not requested become NULL. */
void describe(const hhmm_request *r, const hhmm_result *o, hhmm_request *dr, hhmm_result *dq,
              std::vector<ArrayDesc> &v);

/* One shard of a host request: per array class (series, draws, pairs) the
 * first element, the element count and the caller's leading extent.  An
 * array of class c with e elements is then `e / lead` rows of `cnt` elements,
 * at a pitch of `lead` in the caller's buffer and packed in the shard's
 * device copy -- which is exactly the [N', ...] / [S', ...] / [P', ...]
 * layout of the sub-request (every array is series-, draw- or pair-fastest). */
struct Shard {
    int64_t off[3], cnt[3], lead[3];
};
Shard whole_shard(const hhmm_request *r);
std::vector<Shard> make_shards(const hhmm_request *r, int n);
std::vector<Shard> split_shard(const hhmm_request *r, const Shard &sh, int64_t n);
std::vector<Shard> series_ranges(const hhmm_request *r, int64_t a0, int64_t a1, int64_t n);

/* One array's shard in the caller's buffer: `rows` rows of `width` bytes at a
 * pitch of `pitch` bytes from `base`; packed (pitch = width) in the shard's copy. */
struct ShardRows {
    char *base;
    size_t rows, width, pitch;
};
ShardRows shard_rows(const void *host, const ArrayDesc &a, const Shard &sh);
/* A shard's rows packed / unpacked with one memcpy per row: what the self-tests hold gather_chunk against. */
void copy_shard_host(void *packed, const void *host, const ArrayDesc &a, const Shard &sh, bool to_packed);

/* fn(0) on the calling thread and fn(1) .. fn(n - 1) each on a thread of its
 * own; a thread that cannot be started leaves its item to the caller (no
 * exception crosses the C ABI).  Returns when every item is done. */
void run_parallel(size_t n, const std::function<void(size_t)> &fn);

void copy_row(char *dst, const char *src, size_t n);
void par_copy_rows(char *dst, size_t dpitch, const char *src, size_t spitch, size_t width, size_t rows);

/* A chunk: its shard, its sub-request's pairs, and where each array sits in the slot. */
struct ChunkLayout {
    Shard sh;
    std::vector<size_t> off;   /* per array of `arrays`, bytes from the slot base */
    size_t status_off = 0;
    size_t in_end = 0;         /* [0, in_end): uploaded */
    size_t out_begin = 0;      /* [out_begin, total): downloaded */
    size_t total = 0;
    int64_t P = 0;
};
size_t shard_bytes(const ArrayDesc &a, const Shard &sh);
ChunkLayout chunk_layout(const hhmm_request *req, const std::vector<ArrayDesc> &arrays, const Shard &sh, bool ragged);
int64_t chunk_staged_pairs(const hhmm_request *req, const Shard &c);
bool chunk_pairs_agree(const hhmm_request *req, const Shard &c, const ChunkLayout &L);

/* Packs the rows of chunk L's uploaded arrays from the caller's buffers into
 * the slot at `dst`. */
void gather_chunk(const std::vector<ArrayDesc> &arrays, const ChunkLayout &L, void *dst);
/* Writes chunk L's downloaded region `src` (the slot from L.out_begin on)
 * into the caller's output arrays and, unless NULL, into `status`, the [P]
 * pair statuses of the whole request of P_request pairs.  Returns the number
 * of non-zero pair statuses. */
int64_t scatter_chunk(const std::vector<ArrayDesc> &arrays, const ChunkLayout &L, const void *src, int32_t *status,
                      int64_t P_request);
int64_t count_nonzero(const int32_t *q, int64_t n);
/* The chunk's sub-request: *cr / *cq are dreq / dres (describe's) with the
 * chunk's n_series and n_draws, and every array and pair_status at its place
 * in the slot at `slot_base` (a device pointer: never dereferenced here). */
void bind_chunk(const std::vector<ArrayDesc> &arrays, const ChunkLayout &L, void *slot_base, const hhmm_request &dreq,
                const hhmm_result &dres, hhmm_request &cr, hhmm_result &cq);

} // namespace hhmm
