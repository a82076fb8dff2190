// snk_bzip2.hip -- bzip2 compressed SIZES on gfx950: len(bz2.compress(s)) at level 9 (libbz2 1.0.8), bit-exact.
//
// Replaces, for the batched path, the codec call of ref:snacc/pairwise_ncd.py (bz2.compress(sequence)); the 33 of
// sys.getsizeof is added in Python.  How the work is organised:
//  * the size is a function of the data alone: the BWT's last column is unique even where rotations tie (tied
//    rotations end in the same byte), MTF / RUNA-RUNB / the table choice are deterministic, and the CRCs and origPtr
//    have fixed widths.  So   size = 4 + ceil((sum of block bits + 80) / 8).
//  * RLE1 and the block cut run on the host, per resident sequence, once (snk_bzip2_prepare): the RLE1 bytes, the
//    unit ends, the raw start of the last block and the first / last runs are kept.  A run pending when a block
//    fills is NOT flushed into it: it is the next block's first unit (the codec's own behaviour; tests/bz2_model.py).
//  * a pair x+y shares x's blocks before x's last one bit for bit (RLE1 runs from the first byte); the pair's own
//    blocks are   x's RLE1 from its last block to its final run  +  RLE1 of the final run merged with y's first run
//    +  y's RLE1 after its first run,   cut again at NBLOCK_MAX.  Singles keep the bits of the blocks before their
//    last one; a pair adds the bits of its own blocks.
//  * the device computes the bits of a batch of blocks: BWT by prefix doubling over cyclic rotations (8 packed bytes,
//    then (rank[i], rank[i+h]) keys, hipcub radix sorts; it stops when every rank is distinct or the prefix covers the
//    block), the last column, then one workgroup per block for MTF, the table choice (groups spread over the
//    threads) and the bit count (snk_bzip2.hip.h).
#include "snk_internal.h"
#include "snacc_hip.h"

#include <hipcub/hipcub.hpp>

#include "snk_bzip2.hip.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {

#define BCHK(c, call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            char m_[384];                                                                    \
            snprintf(m_, sizeof m_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return snk_internal_fail((c), SNK_E_HIP, m_);                                    \
        }                                                                                    \
    } while (0)

// Positions of one device batch: about 48 blocks of 900 k RLE1 bytes, ~44 B of scratch per position (~2.1 GB).
constexpr size_t BZ_BATCH_POS = (size_t)48 * BZ_BLOCK_CAP;
constexpr uint32_t BZ_MAX_BATCH_BLOCKS = 4096;        // block ids take 12 bits of the doubling keys

// ---- host: RLE1 ------------------------------------------------------------------------------------------------------
// Appends the RLE1 units of `n` copies of byte `ch` (a run, cut every 255): 1-3 bytes as they are, 4-255 as 4 bytes
// plus (length - 4).  uend marks the last byte of every unit (one bit per RLE1 byte).
struct BzBits {
    std::vector<uint64_t> w;
    size_t n = 0;
    void push(bool b)
    {
        if ((n & 63) == 0) w.push_back(0);
        if (b) w.back() |= 1ull << (n & 63);
        ++n;
    }
    bool operator[](size_t i) const { return (w[i >> 6] >> (i & 63)) & 1; }
    void clear() { w.clear(); n = 0; }
};

void rle_run(uint8_t ch, size_t n, std::vector<uint8_t> &out, BzBits &uend)
{
    while (n > 0) {
        const size_t k = n < 255 ? n : 255;
        if (k < 4) {
            for (size_t i = 0; i < k; ++i) { out.push_back(ch); uend.push(i + 1 == k); }
        } else {
            for (int i = 0; i < 4; ++i) { out.push_back(ch); uend.push(false); }
            out.push_back((uint8_t)(k - 4)); uend.push(true);
        }
        n -= k;
    }
}

struct BzSeq {
    uint32_t len = 0;
    std::vector<uint8_t> rle;             // RLE1 bytes of the whole sequence
    BzBits uend;                          // ... and its unit ends
    std::vector<uint32_t> bstart;         // RLE1 offset where each block begins
    uint32_t last_rle = 0;                // = bstart.back(): the last block (a pair recomputes from here)
    uint32_t tail_rle = 0;                // RLE1 offset of the final run's units (at or behind last_rle)
    uint32_t tail_len = 0;                // raw bytes of the final run from there
    uint8_t tail_ch = 0;
    uint32_t head_len = 0;                // raw length of the first maximal run
    uint32_t head_rle = 0;                // RLE1 offset behind the first run's units
    uint8_t head_ch = 0;
    uint64_t kept_bits = 0;               // bits of every block before the last one (singles pass)
    uint32_t single = 0;                  // len(bz2.compress(s))
};

// RLE1 of one sequence plus the block cut and the run bookkeeping a pair job needs.
void rle_sequence(const uint8_t *a, uint32_t n, BzSeq &q)
{
    q.len = n;
    q.rle.clear(); q.uend.clear(); q.bstart.clear();
    q.rle.reserve(n + 16); q.uend.w.reserve(n / 64 + 2);
    size_t i = 0, last_run_start = 0, last_run_rle = 0;
    while (i < n) {
        size_t j = i + 1;
        while (j < n && a[j] == a[i]) ++j;
        if (i == 0) { q.head_len = (uint32_t)j; q.head_ch = a[0]; }
        last_run_start = i; last_run_rle = q.rle.size();
        rle_run(a[i], j - i, q.rle, q.uend);
        if (i == 0) q.head_rle = (uint32_t)q.rle.size();
        i = j;
    }
    // the block cut: after the unit that brings a block to NBLOCK_MAX bytes; no empty block at the end
    const size_t m = q.rle.size();
    size_t b = 0;
    while (b < m) {
        q.bstart.push_back((uint32_t)b);
        size_t e = b + BZ_NBLOCK_MAX - 1;
        if (e >= m - 1) break;
        while (!q.uend[e]) ++e;
        b = e + 1;
    }
    q.rle.shrink_to_fit();
    q.last_rle = q.bstart.empty() ? 0u : q.bstart.back();
    // the final run from the last block on: its 255-chunks before last_rle stay in the kept blocks
    if (n) {
        q.tail_ch = a[n - 1];
        size_t r = last_run_rle, raw = last_run_start;
        while (r < q.last_rle) {                 // whole 255-chunks of the final run that sit in earlier blocks
            r += 5; raw += 255;
        }
        q.tail_rle = (uint32_t)r;
        q.tail_len = (uint32_t)(n - raw);
    }
}

// ---- device: BWT by prefix doubling ----------------------------------------------------------------------------------
__global__ void bz_bid_kernel(const uint32_t *__restrict__ boff, uint32_t *__restrict__ bid)
{
    const uint32_t b = blockIdx.x;
    for (uint32_t p = boff[b] + threadIdx.x; p < boff[b + 1]; p += blockDim.x) bid[p] = b;
}

__device__ __forceinline__ uint64_t bz_key8(const uint8_t *blk, uint32_t base, uint32_t n, uint32_t i)
{
    uint64_t k = 0;
    for (int t = 0; t < 8; ++t) {
        uint32_t j = i + t;
        while (j >= n) j -= n;                   // cyclic: blocks shorter than 8 wrap more than once
        k = (k << 8) | blk[base + j];
    }
    return k;
}

__global__ void bz_key0_kernel(const uint8_t *__restrict__ blk, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ bid,
                               uint32_t total, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const uint32_t b = bid[p], base = boff[b], n = boff[b + 1] - base;
        key[p] = bz_key8(blk, base, n, p - base);
        val[p] = p;
    }
}

__global__ void bz_keybid_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ bid, uint32_t total, uint64_t *__restrict__ key)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) key[k] = bid[sa[k]];
}

// hv[k] = k where sorted position k starts a new group (block or 8-byte key differs), else 0; counts the heads.
__global__ void bz_head0_kernel(const uint8_t *__restrict__ blk, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ bid,
                                const uint32_t *__restrict__ sa, uint32_t total, uint32_t *__restrict__ hv, uint32_t *__restrict__ nheads)
{
    uint32_t cnt = 0;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
        bool head = k == 0;
        if (!head) {
            const uint32_t p = sa[k], q = sa[k - 1], b = bid[p];
            if (bid[q] != b) head = true;
            else {
                const uint32_t base = boff[b], n = boff[b + 1] - base;
                head = bz_key8(blk, base, n, p - base) != bz_key8(blk, base, n, q - base);
            }
        }
        hv[k] = head ? k : 0u;
        cnt += head;
    }
    if (cnt) atomicAdd(nheads, cnt);
}

__global__ void bz_head_kernel(const uint64_t *__restrict__ skey, uint32_t total, uint32_t *__restrict__ hv, uint32_t *__restrict__ nheads)
{
    uint32_t cnt = 0;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
        const bool head = k == 0 || skey[k] != skey[k - 1];
        hv[k] = head ? k : 0u;
        cnt += head;
    }
    if (cnt) atomicAdd(nheads, cnt);
}

// rank of a position = sorted index of its group's head, relative to its block (< 2^20)
__global__ void bz_rank_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ hd, const uint32_t *__restrict__ boff,
                               const uint32_t *__restrict__ bid, uint32_t total, uint32_t *__restrict__ rank)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
        const uint32_t p = sa[k];
        rank[p] = hd[k] - boff[bid[p]];
    }
}

__global__ void bz_keyh_kernel(const uint32_t *__restrict__ rank, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ bid,
                               uint32_t total, uint32_t h, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const uint32_t b = bid[p], base = boff[b], n = boff[b + 1] - base;
        uint32_t j = (p - base) + h % n;
        if (j >= n) j -= n;
        key[p] = ((uint64_t)b << 40) | ((uint64_t)rank[p] << 20) | rank[base + j];
        val[p] = p;
    }
}

// BWT last column: the byte before each sorted rotation.
__global__ void bz_last_kernel(const uint8_t *__restrict__ blk, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ bid,
                               const uint32_t *__restrict__ sa, uint32_t total, uint8_t *__restrict__ last)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
        const uint32_t p = sa[k], b = bid[p], base = boff[b], n = boff[b + 1] - base;
        const uint32_t i = p - base;
        last[k] = blk[base + (i == 0 ? n - 1 : i - 1)];
    }
}

// One workgroup per block: MTF in 256 chunks (recency lists per lane, an in-order combine on lane 0, then every lane
// codes its own chunk), the RUNA/RUNB coding placed by a prefix count, then the four refinement passes with the groups
// spread over the lanes, the code lengths (one lane per table, work arrays in LDS) and the bit count.  The BWT last
// column is overwritten with the MTF positions.  mtfv: n + 1 slots per block at boff[b] + b.
constexpr int BZ_STAGE_THREADS = 256;
__global__ void __launch_bounds__(BZ_STAGE_THREADS)
bz_stage_kernel(uint8_t *__restrict__ last, const uint32_t *__restrict__ boff, uint16_t *__restrict__ mtfv_all,
                uint64_t *__restrict__ bits_out)
{
    __shared__ BzTables tb;
    __shared__ uint8_t sel[BZ_MAX_SEL];
    __shared__ uint8_t lists[BZ_STAGE_THREADS][256];          // per chunk: its recency list, then its starting MTF list
    __shared__ int32_t hbwork[BZ_N_GROUPS][BZ_HB_WORK];
    __shared__ uint8_t used[256], seq_of[256], cur[256], prev[256], tmp[256];
    __shared__ uint32_t freq[BZ_MAX_ALPHA];
    __shared__ int cnt[BZ_STAGE_THREADS];
    __shared__ int s_nin, s_nmtf, s_used16;
    const uint32_t b = blockIdx.x, base = boff[b], n = boff[b + 1] - base;
    uint8_t *L = last + base;
    uint16_t *mtfv = mtfv_all + base + b;
    const int tid = threadIdx.x;
    used[tid] = 0;
    if (tid < BZ_MAX_ALPHA) freq[tid] = 0;
    if (tid < BZ_MAX_ALPHA - BZ_STAGE_THREADS) freq[BZ_STAGE_THREADS + tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += BZ_STAGE_THREADS) {
        const uint8_t c = L[i];
        if (!used[c]) used[c] = 1;
    }
    __syncthreads();
    if (tid == 0) {
        int n_in_use = 0, used16 = 0;
        for (int i = 0; i < 256; i++)
            if (used[i]) seq_of[i] = (uint8_t)n_in_use++;
        for (int i = 0; i < 16; i++) {
            int u = 0;
            for (int j = 0; j < 16; j++) u |= used[i * 16 + j];
            used16 += u;
        }
        s_nin = n_in_use; s_used16 = used16;
    }
    __syncthreads();
    const int n_in_use = s_nin;
    const int lo = (int)((uint64_t)n * tid / BZ_STAGE_THREADS), hi = (int)((uint64_t)n * (tid + 1) / BZ_STAGE_THREADS);
    cnt[tid] = bz_mtf_recency(L, lo, hi, seq_of, lists[tid]);
    __syncthreads();
    if (tid == 0) {                                            // starting list of every chunk
        for (int i = 0; i < n_in_use; i++) cur[i] = (uint8_t)i;
        for (int c = 0; c < BZ_STAGE_THREADS; c++) {
            for (int i = 0; i < n_in_use; i++) prev[i] = cur[i];
            bz_mtf_combine(cur, lists[c], cnt[c], n_in_use, tmp);
            for (int i = 0; i < n_in_use; i++) lists[c][i] = prev[i];
        }
    }
    __syncthreads();
    bz_mtf_positions(L, lo, hi, seq_of, lists[tid], L);
    __syncthreads();
    cnt[tid] = bz_mtf_code_chunk(L, lo, hi, (int)n, nullptr, nullptr);
    __syncthreads();
    if (tid == 0) {                                            // exclusive prefix of the symbol counts
        int acc = 0;
        for (int c = 0; c < BZ_STAGE_THREADS; c++) { const int k = cnt[c]; cnt[c] = acc; acc += k; }
        mtfv[acc] = (uint16_t)(n_in_use + 1);                  // EOB
        s_nmtf = acc + 1;
    }
    __syncthreads();
    bz_mtf_code_chunk(L, lo, hi, (int)n, mtfv + cnt[tid], nullptr);
    __syncthreads();
    const int n_mtf = s_nmtf, alpha = n_in_use + 2, ng = bz_n_groups(n_mtf);
    for (int i = tid; i < n_mtf; i += BZ_STAGE_THREADS) atomicAdd(&freq[mtfv[i]], 1u);
    __syncthreads();
    if (tid == 0) {
        for (int t = 0; t < BZ_N_GROUPS; t++)
            for (int v = 0; v < alpha; v++) tb.len[t][v] = 15;
        bz_initial_tables(freq, alpha, n_mtf, ng, tb.len);
    }
    __syncthreads();
    const int n_sel = (n_mtf + BZ_G_SIZE - 1) / BZ_G_SIZE;
    for (int it = 0; it < BZ_N_ITERS; it++) {
        for (int i = tid; i < BZ_N_GROUPS * BZ_MAX_ALPHA; i += BZ_STAGE_THREADS) (&tb.rfreq[0][0])[i] = 0;
        __syncthreads();
        for (int g = tid; g < n_sel; g += BZ_STAGE_THREADS) {
            const int bt = bz_best_table(mtfv, n_mtf, g, ng, tb.len);
            sel[g] = (uint8_t)bt;
            const int gs = g * BZ_G_SIZE, ge = gs + BZ_G_SIZE < n_mtf ? gs + BZ_G_SIZE : n_mtf;
            for (int i = gs; i < ge; i++) atomicAdd(&tb.rfreq[bt][mtfv[i]], 1);
        }
        __syncthreads();
        if (tid < ng) bz_make_code_lengths(tb.len[tid], tb.rfreq[tid], alpha, BZ_MAX_LEN, hbwork[tid]);
        __syncthreads();
    }
    if (tid == 0) bits_out[b] = bz_tail_bits(sel, n_sel, ng, tb, alpha, s_used16);
}

// ---- the add-on's state ---------------------------------------------------------------------------------------------
struct BzState {
    int n = 0;
    bool prepared = false, singles_done = false;
    std::vector<BzSeq> seq;
    // device scratch of one batch
    size_t cap_pos = 0, cap_blk = 0;
    uint8_t *d_blk = nullptr, *d_last = nullptr;
    uint32_t *d_boff = nullptr, *d_bid = nullptr, *d_val = nullptr, *d_sa = nullptr, *d_rank = nullptr, *d_hv = nullptr, *d_hd = nullptr;
    uint32_t *d_nheads = nullptr;
    uint64_t *d_key = nullptr, *d_skey = nullptr, *d_bits = nullptr;
    uint16_t *d_mtfv = nullptr;
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    uint8_t *h_blk = nullptr;                 // pinned staging of one batch's block bytes
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    uint32_t *h_out = nullptr; size_t out_cap = 0;   // pinned source of snk_bzip2_pairs_device's copy
    hipEvent_t out_busy = nullptr;                   // ... recorded behind that copy
};

void bz_free_scratch(BzState *s)
{
    for (void *p : {(void *)s->d_blk, (void *)s->d_last, (void *)s->d_boff, (void *)s->d_bid, (void *)s->d_val, (void *)s->d_sa,
                    (void *)s->d_rank, (void *)s->d_hv, (void *)s->d_hd, (void *)s->d_nheads, (void *)s->d_key, (void *)s->d_skey,
                    (void *)s->d_bits, (void *)s->d_mtfv, s->d_tmp})
        if (p) (void)hipFree(p);
    if (s->h_blk) (void)hipHostFree(s->h_blk);
    s->d_blk = s->d_last = nullptr; s->d_boff = s->d_bid = s->d_val = s->d_sa = s->d_rank = s->d_hv = s->d_hd = s->d_nheads = nullptr;
    s->d_key = s->d_skey = s->d_bits = nullptr; s->d_mtfv = nullptr; s->d_tmp = nullptr; s->h_blk = nullptr;
    s->cap_pos = s->cap_blk = 0; s->tmp_bytes = 0;
}

void bz_destroy(void *p)
{
    BzState *s = (BzState *)p;
    if (!s) return;
    bz_free_scratch(s);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->out_busy) { (void)hipEventSynchronize(s->out_busy); (void)hipEventDestroy(s->out_busy); }
    if (s->h_out) (void)hipHostFree(s->h_out);
    delete s;
}

int bz_ensure_scratch(snk_ctx *c, BzState *s, const SnkSeqView &v, size_t pos, size_t nblk)
{
    if (pos <= s->cap_pos && nblk <= s->cap_blk) return SNK_OK;
    bz_free_scratch(s);
    pos = std::max(pos, (size_t)BZ_BLOCK_CAP);
    nblk = std::max<size_t>(nblk, 64);
    BCHK(c, hipMalloc((void **)&s->d_blk, pos));
    BCHK(c, hipMalloc((void **)&s->d_last, pos));
    BCHK(c, hipMalloc((void **)&s->d_boff, (nblk + 1) * 4));
    BCHK(c, hipMalloc((void **)&s->d_bid, pos * 4));
    BCHK(c, hipMalloc((void **)&s->d_val, pos * 4));
    BCHK(c, hipMalloc((void **)&s->d_sa, pos * 4));
    BCHK(c, hipMalloc((void **)&s->d_rank, pos * 4));
    BCHK(c, hipMalloc((void **)&s->d_hv, pos * 4));
    BCHK(c, hipMalloc((void **)&s->d_hd, pos * 4));
    BCHK(c, hipMalloc((void **)&s->d_nheads, 4));
    BCHK(c, hipMalloc((void **)&s->d_key, pos * 8));
    BCHK(c, hipMalloc((void **)&s->d_skey, pos * 8));
    BCHK(c, hipMalloc((void **)&s->d_bits, nblk * 8));
    BCHK(c, hipMalloc((void **)&s->d_mtfv, (pos + nblk) * 2));
    BCHK(c, hipHostMalloc((void **)&s->h_blk, pos, hipHostMallocDefault));
    size_t t1 = 0, t2 = 0;
    BCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, t1, s->d_key, s->d_skey, s->d_val, s->d_sa, (int)pos, 0, 64, v.stream));
    BCHK(c, hipcub::DeviceScan::InclusiveScan(nullptr, t2, s->d_hv, s->d_hd, hipcub::Max(), (int)pos, v.stream));
    s->tmp_bytes = std::max(t1, t2);
    BCHK(c, hipMalloc(&s->d_tmp, s->tmp_bytes ? s->tmp_bytes : 16));
    s->cap_pos = pos; s->cap_blk = nblk;
    return SNK_OK;
}

inline unsigned grid_for(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 8192); }

// Bits of the blocks staged in s->h_blk (offsets hoff[0..nb]) -> bits[0..nb).  Device time goes to *ms.
int bz_run_batch(snk_ctx *c, BzState *s, const SnkSeqView &v, const std::vector<uint32_t> &hoff, uint64_t *bits, double *ms)
{
    const uint32_t nb = (uint32_t)hoff.size() - 1, total = hoff[nb];
    if (nb == 0) return SNK_OK;
    hipStream_t st = v.stream;
    uint32_t maxlen = 0;
    for (uint32_t b = 0; b < nb; ++b) maxlen = std::max(maxlen, hoff[b + 1] - hoff[b]);
    BCHK(c, hipMemcpyAsync(s->d_blk, s->h_blk, total, hipMemcpyHostToDevice, st));
    BCHK(c, hipMemcpyAsync(s->d_boff, hoff.data(), (nb + 1) * 4, hipMemcpyHostToDevice, st));
    BCHK(c, hipEventRecord(s->ev0, st));
    hipLaunchKernelGGL(bz_bid_kernel, dim3(nb), dim3(256), 0, st, s->d_boff, s->d_bid);
    hipLaunchKernelGGL(bz_key0_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_blk, s->d_boff, s->d_bid, total, s->d_key, s->d_val);
    // sort by the 8 bytes, then (stable) by block
    BCHK(c, hipcub::DeviceRadixSort::SortPairs(s->d_tmp, s->tmp_bytes, s->d_key, s->d_skey, s->d_val, s->d_sa, (int)total, 0, 64, st));
    hipLaunchKernelGGL(bz_keybid_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_sa, s->d_bid, total, s->d_key);
    BCHK(c, hipcub::DeviceRadixSort::SortPairs(s->d_tmp, s->tmp_bytes, s->d_key, s->d_skey, s->d_sa, s->d_val, (int)total, 0, 12, st));
    std::swap(s->d_sa, s->d_val);
    BCHK(c, hipMemsetAsync(s->d_nheads, 0, 4, st));
    hipLaunchKernelGGL(bz_head0_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_blk, s->d_boff, s->d_bid, s->d_sa, total, s->d_hv, s->d_nheads);
    uint32_t heads = 0;
    uint32_t cover = 8;
    while (true) {
        BCHK(c, hipcub::DeviceScan::InclusiveScan(s->d_tmp, s->tmp_bytes, s->d_hv, s->d_hd, hipcub::Max(), (int)total, st));
        hipLaunchKernelGGL(bz_rank_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_sa, s->d_hd, s->d_boff, s->d_bid, total, s->d_rank);
        BCHK(c, hipMemcpyAsync(&heads, s->d_nheads, 4, hipMemcpyDeviceToHost, st));
        BCHK(c, hipStreamSynchronize(st));
        // every rotation distinct, or the compared prefix covers every block (whole-block periodic inputs tie for good)
        if (heads >= total || cover >= maxlen) break;
        hipLaunchKernelGGL(bz_keyh_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_rank, s->d_boff, s->d_bid, total, cover, s->d_key, s->d_val);
        BCHK(c, hipcub::DeviceRadixSort::SortPairs(s->d_tmp, s->tmp_bytes, s->d_key, s->d_skey, s->d_val, s->d_sa, (int)total, 0, 52, st));
        BCHK(c, hipMemsetAsync(s->d_nheads, 0, 4, st));
        hipLaunchKernelGGL(bz_head_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_skey, total, s->d_hv, s->d_nheads);
        cover *= 2;
    }
    hipLaunchKernelGGL(bz_last_kernel, dim3(grid_for(total)), dim3(256), 0, st, s->d_blk, s->d_boff, s->d_bid, s->d_sa, total, s->d_last);
    hipLaunchKernelGGL(bz_stage_kernel, dim3(nb), dim3(BZ_STAGE_THREADS), 0, st, s->d_last, s->d_boff, s->d_mtfv, s->d_bits);
    BCHK(c, hipGetLastError());
    BCHK(c, hipEventRecord(s->ev1, st));
    BCHK(c, hipMemcpyAsync(bits, s->d_bits, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    BCHK(c, hipStreamSynchronize(st));
    float t = 0.f;
    BCHK(c, hipEventElapsedTime(&t, s->ev0, s->ev1));
    *ms += t;
    return SNK_OK;
}

// A block to price: where its bytes come from.  Up to three pieces: a slice of x's RLE1, the merged run, a slice of
// y's RLE1 (a single's block is one slice).
struct BzPiece { const uint8_t *p; uint32_t n; };
struct BzBlock { uint32_t job; BzPiece part[3]; uint32_t len; };

int bz_price(snk_ctx *c, BzState *s, const SnkSeqView &v, const std::vector<BzBlock> &blocks, std::vector<uint64_t> &job_bits, double *ms)
{
    size_t i = 0;
    std::vector<uint32_t> hoff;
    std::vector<uint64_t> bits;
    while (i < blocks.size()) {
        size_t j = i, tot = 0;
        while (j < blocks.size() && j - i < BZ_MAX_BATCH_BLOCKS && (j == i || tot + blocks[j].len <= BZ_BATCH_POS)) tot += blocks[j++].len;
        int rc = bz_ensure_scratch(c, s, v, std::max(tot, std::min(BZ_BATCH_POS, (size_t)BZ_BLOCK_CAP * 8)), std::max<size_t>(j - i, 256));
        if (rc != SNK_OK) return rc;
        hoff.assign(1, 0);
        for (size_t k = i; k < j; ++k) {
            uint8_t *dst = s->h_blk + hoff.back();
            for (const BzPiece &pc : blocks[k].part)
                if (pc.n) { memcpy(dst, pc.p, pc.n); dst += pc.n; }
            hoff.push_back(hoff.back() + blocks[k].len);
        }
        bits.assign(j - i, 0);
        rc = bz_run_batch(c, s, v, hoff, bits.data(), ms);
        if (rc != SNK_OK) return rc;
        for (size_t k = i; k < j; ++k) job_bits[blocks[k].job] += bits[k - i];
        i = j;
    }
    return SNK_OK;
}

inline uint32_t stream_size(uint64_t bits) { return (uint32_t)(4 + (bits + 80 + 7) / 8); }

// Cut a virtual stream (up to three pieces, with their unit-end flags) into blocks for job `job`.
struct BzUend { const BzBits *bits; size_t off; };
void bz_cut(uint32_t job, const BzPiece (&pc)[3], const BzUend (&ue)[3], std::vector<BzBlock> &out)
{
    uint64_t total = 0;
    for (const BzPiece &p : pc) total += p.n;
    uint64_t b = 0;
    auto uend_at = [&](uint64_t q) -> bool {
        for (int k = 0; k < 3; ++k) {
            if (q < pc[k].n) return (*ue[k].bits)[ue[k].off + q];
            q -= pc[k].n;
        }
        return true;
    };
    while (b < total) {
        uint64_t e = b + BZ_NBLOCK_MAX - 1;
        if (e >= total - 1) e = total - 1;
        else
            while (!uend_at(e)) ++e;
        BzBlock blk{};
        blk.job = job;
        blk.len = (uint32_t)(e + 1 - b);
        uint64_t off = 0;
        int np = 0;
        for (int k = 0; k < 3; ++k) {               // the intersection of [b, e] with each piece
            const uint64_t lo = std::max<uint64_t>(b, off), hi = std::min<uint64_t>(e + 1, off + pc[k].n);
            if (lo < hi) blk.part[np++] = BzPiece{pc[k].p + (lo - off), (uint32_t)(hi - lo)};
            off += pc[k].n;
        }
        out.push_back(blk);
        b = e + 1;
    }
}

int bz_get(snk_ctx *c, SnkSeqView &v, BzState *&s)
{
    int rc = snk_internal_view(c, &v);
    if (rc != SNK_OK) return rc;
    if (v.n <= 0) return snk_internal_fail(c, SNK_E_STATE, "no sequences resident (call snk_upload first)");
    void (**free_fn)(void *) = nullptr;
    void **slot = snk_internal_bz_slot(c, &free_fn);
    if (!*slot) {
        BzState *ns = new (std::nothrow) BzState();
        if (!ns) return snk_internal_fail(c, SNK_E_HIP, "out of host memory");
        ns->n = v.n;
        if (hipEventCreate(&ns->ev0) != hipSuccess || hipEventCreate(&ns->ev1) != hipSuccess ||
            hipEventCreateWithFlags(&ns->out_busy, hipEventDisableTiming) != hipSuccess) {
            bz_destroy(ns);
            return snk_internal_fail(c, SNK_E_HIP, "hipEventCreate failed");
        }
        *slot = ns; *free_fn = bz_destroy;
    }
    s = (BzState *)*slot;
    return SNK_OK;
}

// RLE1 + block cut of every resident sequence (host threads), from a copy of the device arena.
int bz_prepare(snk_ctx *c, SnkSeqView &v, BzState *&s)
{
    int rc = bz_get(c, v, s);
    if (rc != SNK_OK || s->prepared) return rc;
    const int n = v.n;
    s->seq.assign((size_t)n, BzSeq{});
    // one sequence at a time per host thread: the host holds the RLE1 streams, not a copy of the arena
    std::atomic<int> next{0}, failed{0};
    auto work = [&]() {
        std::vector<uint8_t> host;
        for (int g; (g = next.fetch_add(1)) < n;) {
            host.resize(v.len[g]);
            if (v.len[g] && hipMemcpy(host.data(), v.d_bytes + v.boff[g], v.len[g], hipMemcpyDeviceToHost) != hipSuccess) {
                failed = 1;
                return;
            }
            rle_sequence(host.data(), v.len[g], s->seq[(size_t)g]);
        }
    };
    const int nt = std::max(1, std::min<int>(n, (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()))));
    std::vector<std::thread> ts;
    for (int t = 1; t < nt; ++t) ts.emplace_back(work);
    work();
    for (auto &t : ts) t.join();
    if (failed) return snk_internal_fail(c, SNK_E_HIP, "copying a sequence to the host failed");
    s->prepared = true;
    return SNK_OK;
}

int bz_singles(snk_ctx *c, SnkSeqView &v, BzState *&s)
{
    int rc = bz_prepare(c, v, s);
    if (rc != SNK_OK || s->singles_done) return rc;
    const int n = v.n;
    std::vector<BzBlock> blocks;
    std::vector<uint64_t> kept((size_t)n, 0), lastb((size_t)n, 0);
    // jobs 0..n-1: the blocks before the last one; jobs n..2n-1: the last block
    for (int g = 0; g < n; ++g) {
        const BzSeq &q = s->seq[(size_t)g];
        for (size_t k = 0; k < q.bstart.size(); ++k) {
            const uint32_t b0 = q.bstart[k], b1 = k + 1 < q.bstart.size() ? q.bstart[k + 1] : (uint32_t)q.rle.size();
            BzBlock blk{};
            blk.job = k + 1 < q.bstart.size() ? (uint32_t)g : (uint32_t)(n + g);
            blk.part[0] = BzPiece{q.rle.data() + b0, b1 - b0};
            blk.len = b1 - b0;
            blocks.push_back(blk);
        }
    }
    std::vector<uint64_t> bits((size_t)2 * n, 0);
    double ms = 0;
    rc = bz_price(c, s, v, blocks, bits, &ms);
    if (rc != SNK_OK) return rc;
    for (int g = 0; g < n; ++g) {
        s->seq[(size_t)g].kept_bits = bits[(size_t)g];
        s->seq[(size_t)g].single = stream_size(bits[(size_t)g] + bits[(size_t)n + g]);
    }
    s->singles_done = true;
    return SNK_OK;
}

// Sizes of the pairs (x, y) = ij[2k], ij[2k+1] (y = -1: the single x).
int bz_pairs(snk_ctx *c, int n_pairs, const int32_t *ij, uint32_t *sizes)
{
    SnkSeqView v; BzState *s = nullptr;
    int rc = bz_singles(c, v, s);
    if (rc != SNK_OK) return rc;
    for (int k = 0; k < n_pairs; ++k)
        if (ij[2 * k] < 0 || ij[2 * k] >= v.n || ij[2 * k + 1] < -1 || ij[2 * k + 1] >= v.n)
            return snk_internal_fail(c, SNK_E_ARG, "pair index out of range");
    std::vector<BzBlock> blocks;
    std::vector<std::vector<uint8_t>> mid_bytes((size_t)n_pairs);
    std::vector<BzBits> mid_uend((size_t)n_pairs);
    std::vector<uint64_t> bits((size_t)n_pairs, 0);
    s->last_ms = 0.0;
    // a bounded number of pairs per pass: the merged runs are small, the blocks are only references
    const size_t PASS = 4096;
    for (size_t k0 = 0; k0 < (size_t)n_pairs; k0 += PASS) {
        const size_t k1 = std::min((size_t)n_pairs, k0 + PASS);
        blocks.clear();
        for (size_t k = k0; k < k1; ++k) {
            const BzSeq &x = s->seq[(size_t)ij[2 * k]];
            if (ij[2 * k + 1] < 0) continue;
            const BzSeq &y = s->seq[(size_t)ij[2 * k + 1]];
            bits[k] = x.kept_bits;
            BzPiece pc[3] = {};
            BzUend ue[3] = {{&x.uend, 0}, {&x.uend, 0}, {&x.uend, 0}};
            std::vector<uint8_t> &mb = mid_bytes[k];
            BzBits &mu = mid_uend[k];
            mb.clear(); mu.clear();
            uint32_t ystart = 0;
            if (x.len == 0) {
                pc[2] = BzPiece{y.rle.data(), (uint32_t)y.rle.size()}; ue[2] = BzUend{&y.uend, 0};
            } else {
                pc[0] = BzPiece{x.rle.data() + x.last_rle, x.tail_rle - x.last_rle}; ue[0] = BzUend{&x.uend, x.last_rle};
                size_t run = x.tail_len;
                if (y.len && y.head_ch == x.tail_ch) { run += y.head_len; ystart = y.head_rle; }
                rle_run(x.tail_ch, run, mb, mu);
                pc[1] = BzPiece{mb.data(), (uint32_t)mb.size()}; ue[1] = BzUend{&mu, 0};
                pc[2] = BzPiece{y.rle.data() + ystart, (uint32_t)(y.rle.size() - ystart)}; ue[2] = BzUend{&y.uend, ystart};
            }
            bz_cut((uint32_t)k, pc, ue, blocks);
        }
        rc = bz_price(c, s, v, blocks, bits, &s->last_ms);
        if (rc != SNK_OK) return rc;
    }
    for (size_t k = 0; k < (size_t)n_pairs; ++k)
        sizes[k] = ij[2 * k + 1] < 0 ? s->seq[(size_t)ij[2 * k]].single : stream_size(bits[k]);
    return SNK_OK;
}

int bz_rows(snk_ctx *c, int r0, int r1, std::vector<uint32_t> &out)
{
    SnkSeqView v;
    int rc = snk_internal_view(c, &v);
    if (rc != SNK_OK) return rc;
    if (v.n <= 0) return snk_internal_fail(c, SNK_E_STATE, "no sequences resident (call snk_upload first)");
    if (r0 < 0 || r1 > v.n || r0 > r1) return snk_internal_fail(c, SNK_E_ARG, "row range out of bounds");
    const size_t n = (size_t)v.n, m = (size_t)(r1 - r0) * n;
    std::vector<int32_t> ij(2 * m);
    for (size_t k = 0; k < m; ++k) { ij[2 * k] = r0 + (int32_t)(k / n); ij[2 * k + 1] = (int32_t)(k % n); }
    out.assign(m, 0);
    return m ? bz_pairs(c, (int)m, ij.data(), out.data()) : SNK_OK;
}

}  // namespace

extern "C" {

int snk_bzip2_prepare(snk_ctx *c)
{
    if (!c) return SNK_E_ARG;
    SnkSeqView v; BzState *s = nullptr;
    return bz_prepare(c, v, s);
}

int snk_bzip2_singles(snk_ctx *c, uint32_t *sizes)
{
    if (!c || !sizes) return c ? snk_internal_fail(c, SNK_E_ARG, "sizes is NULL") : SNK_E_ARG;
    SnkSeqView v; BzState *s = nullptr;
    int rc = bz_singles(c, v, s);
    if (rc != SNK_OK) return rc;
    for (int g = 0; g < v.n; ++g) sizes[g] = s->seq[(size_t)g].single;
    return SNK_OK;
}

int snk_bzip2_pairs(snk_ctx *c, int row_begin, int row_end, uint32_t *sizes)
{
    if (!c || !sizes) return c ? snk_internal_fail(c, SNK_E_ARG, "sizes is NULL") : SNK_E_ARG;
    std::vector<uint32_t> out;
    int rc = bz_rows(c, row_begin, row_end, out);
    if (rc != SNK_OK) return rc;
    std::copy(out.begin(), out.end(), sizes);
    return SNK_OK;
}

int snk_bzip2_pairs_list(snk_ctx *c, int n_pairs, const int32_t *ij, uint32_t *sizes)
{
    if (!c || n_pairs < 0 || (n_pairs && (!ij || !sizes))) return c ? snk_internal_fail(c, SNK_E_ARG, "bad pair list") : SNK_E_ARG;
    if (n_pairs == 0) return SNK_OK;
    return bz_pairs(c, n_pairs, ij, sizes);
}

int snk_bzip2_pairs_device(snk_ctx *c, int row_begin, int row_end, void *d_sizes, void *hip_stream)
{
    if (!c || !d_sizes) return c ? snk_internal_fail(c, SNK_E_ARG, "d_sizes is NULL") : SNK_E_ARG;
    std::vector<uint32_t> out;
    int rc = bz_rows(c, row_begin, row_end, out);
    if (rc != SNK_OK) return rc;
    SnkSeqView v; BzState *s = nullptr;
    rc = bz_get(c, v, s);
    if (rc != SNK_OK) return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : v.stream;
    // the sizes are known on the host by now; their copy is queued on the caller's stream and not waited for (snk_sync).
    // The pinned source is reused only after the previous call's copy has left it.
    BCHK(c, hipEventSynchronize(s->out_busy));
    if (out.size() > s->out_cap) {
        if (s->h_out) BCHK(c, hipHostFree(s->h_out));
        s->h_out = nullptr; s->out_cap = 0;
        BCHK(c, hipHostMalloc((void **)&s->h_out, out.size() * 4, hipHostMallocDefault));
        s->out_cap = out.size();
    }
    if (out.empty()) return SNK_OK;
    memcpy(s->h_out, out.data(), out.size() * 4);
    BCHK(c, hipMemcpyAsync(d_sizes, s->h_out, out.size() * 4, hipMemcpyHostToDevice, st));
    BCHK(c, hipEventRecord(s->out_busy, st));
    return SNK_OK;
}

double snk_bzip2_last_ms(snk_ctx *c)
{
    if (!c) return -1.0;
    void **slot = snk_internal_bz_slot(c, nullptr);
    return *slot ? ((BzState *)*slot)->last_ms : 0.0;
}

}  // extern "C"
