// snk_bzip2.hip.h -- the per-block stages of the bzip2 size path: MTF with the RUNA/RUNB
// zero-run coding, the table choice of libbz2 1.0.8's sendMTFValues, BZ2_hbMakeCodeLengths (maxLen 17) and the bit
// count of a block.  Every function is __host__ __device__ and needs nothing but <stdint.h>, so g++ compiles this
// header into the CPU test (tests/test_bzip2_model.py) and the kernels in snk_bzip2.hip call the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif

#define BZ_LEVEL 9
#define BZ_NBLOCK_MAX (100000 * BZ_LEVEL - 19)     // a block is cut once it holds this many RLE1 bytes
#define BZ_BLOCK_CAP (BZ_NBLOCK_MAX + 4)            // the unit that crosses the limit adds at most 4 more
#define BZ_MAX_ALPHA 258
#define BZ_N_GROUPS 6
#define BZ_G_SIZE 50
#define BZ_N_ITERS 4
#define BZ_MAX_LEN 17
#define BZ_MAX_SEL ((BZ_BLOCK_CAP + 1 + BZ_G_SIZE - 1) / BZ_G_SIZE)
// fixed bits of a block: magic (48), block CRC (32), randomised (1), origPtr (24), the 16-bit used map, nGroups (3),
// nSelectors (15)
#define BZ_BLOCK_FIXED_BITS (48 + 32 + 1 + 24 + 16 + 3 + 15)

// Tables of one block under choice: code lengths per table, symbol frequencies per table of the last pass.
struct BzTables {
    uint8_t len[BZ_N_GROUPS][BZ_MAX_ALPHA];
    int32_t rfreq[BZ_N_GROUPS][BZ_MAX_ALPHA];
};

// MTF of a BWT last column `last[0..n)` with the RUNA (0) / RUNB (1) coding of zero runs; `seq_of` maps a byte to its
// rank among the used bytes (nInUse of them).  Writes mtfv (at most n + 1 values, EOB = nInUse + 1 last), adds the
// symbol frequencies to freq[0..nInUse+2) (zeroed by the caller) and returns nMTF.
BZ_HD inline int bz_mtf(const uint8_t *last, int n, const uint8_t *seq_of, int n_in_use, uint16_t *mtfv, uint32_t *freq)
{
    uint8_t yy[256];
    for (int i = 0; i < n_in_use; i++) yy[i] = (uint8_t)i;
    int wr = 0;
    uint32_t z = 0;
    for (int i = 0; i <= n; i++) {
        const bool end = i == n;
        uint8_t s = end ? 0 : seq_of[last[i]];
        if (!end && yy[0] == s) { z++; continue; }
        if (z > 0) {
            z--;
            while (true) {
                uint16_t r = (z & 1) ? 1 : 0;
                mtfv[wr++] = r; freq[r]++;
                if (z < 2) break;
                z = (z - 2) / 2;
            }
            z = 0;
        }
        if (end) break;
        uint8_t tmp = yy[1], tmp2;
        yy[1] = yy[0];
        int j = 1;
        while (s != tmp) { j++; tmp2 = tmp; tmp = yy[j]; yy[j] = tmp2; }
        yy[0] = tmp;
        mtfv[wr++] = (uint16_t)(j + 1); freq[j + 1]++;
    }
    mtfv[wr++] = (uint16_t)(n_in_use + 1); freq[n_in_use + 1]++;
    return wr;
}

// ---- MTF in chunks (the kernel's form: one chunk per lane) -------------------------------------------------------------
// The MTF list after a chunk is the chunk's distinct symbols by most recent occurrence, then the symbols of the list before
// the chunk that the chunk did not use, in their old order.  So the lists at the chunk starts follow from a per-chunk
// recency list by an in-order combine, and every chunk can then be coded from its own starting list.

// Recency list of last[lo..hi) (ranks via seq_of, most recent first) -> rec; returns its length.
BZ_HD inline int bz_mtf_recency(const uint8_t *last, int lo, int hi, const uint8_t *seq_of, uint8_t *rec)
{
    uint64_t seen[4] = {0, 0, 0, 0};
    int k = 0;
    for (int i = hi - 1; i >= lo; i--) {
        const uint8_t s = seq_of[last[i]];
        const uint64_t bit = 1ull << (s & 63);
        if (!(seen[s >> 6] & bit)) { seen[s >> 6] |= bit; rec[k++] = s; }
    }
    return k;
}

// cur (n_in_use ranks) becomes the list after a chunk with recency list rec[0..k): rec, then cur without rec's symbols.
BZ_HD inline void bz_mtf_combine(uint8_t *cur, const uint8_t *rec, int k, int n_in_use, uint8_t *tmp)
{
    uint64_t in_rec[4] = {0, 0, 0, 0};
    for (int i = 0; i < k; i++) { tmp[i] = rec[i]; in_rec[rec[i] >> 6] |= 1ull << (rec[i] & 63); }
    int w = k;
    for (int i = 0; i < n_in_use; i++)
        if (!(in_rec[cur[i] >> 6] & (1ull << (cur[i] & 63)))) tmp[w++] = cur[i];
    for (int i = 0; i < n_in_use; i++) cur[i] = tmp[i];
}

// MTF positions of last[lo..hi) from the starting list yy (updated in place): pos[i] = 0 where the symbol is already in
// front (a zero run), else its list position j >= 1.  pos may alias last (each byte is read before it is written).
BZ_HD inline void bz_mtf_positions(const uint8_t *last, int lo, int hi, const uint8_t *seq_of, uint8_t *yy, uint8_t *pos)
{
    for (int i = lo; i < hi; i++) {
        const uint8_t s = seq_of[last[i]];
        if (yy[0] == s) { pos[i] = 0; continue; }
        uint8_t tmp = yy[1], tmp2;
        yy[1] = yy[0];
        int j = 1;
        while (s != tmp) { j++; tmp2 = tmp; tmp = yy[j]; yy[j] = tmp2; }
        yy[0] = tmp;
        pos[i] = (uint8_t)j;
    }
}

// Symbols of the RUNA/RUNB coding of a zero run of length z (bijective base 2): floor(log2(z + 1)).
BZ_HD inline int bz_run_symbols(uint32_t z)
{
    int c = 0;
    for (uint32_t v = z + 1; v > 1; v >>= 1) c++;
    return c;
}

// The mtfv symbols that positions pos[lo..hi) own: every non-zero position is one symbol (j + 1); a zero run belongs to
// the chunk it starts in, even where it runs on past hi.  out == nullptr: count only.  Adds to freq (if given) when
// writing.
BZ_HD inline int bz_mtf_code_chunk(const uint8_t *pos, int lo, int hi, int n, uint16_t *out, uint32_t *freq)
{
    int w = 0;
    for (int i = lo; i < hi; i++) {
        if (pos[i]) {
            if (out) { out[w] = (uint16_t)(pos[i] + 1); if (freq) freq[pos[i] + 1]++; }
            w++;
            continue;
        }
        if (i > 0 && pos[i - 1] == 0) continue;                 // inside a run started earlier
        int e = i + 1;
        while (e < n && pos[e] == 0) e++;
        uint32_t z = (uint32_t)(e - i);
        if (!out) { w += bz_run_symbols(z); continue; }
        z--;
        while (true) {
            const uint16_t r = (z & 1) ? 1 : 0;
            out[w++] = r;
            if (freq) freq[r]++;
            if (z < 2) break;
            z = (z - 2) / 2;
        }
    }
    return w;
}

// The chunked MTF run serially over `chunks` chunks (what the kernel does with one chunk per lane); same result as
// bz_mtf.  pos: n bytes of scratch.
BZ_HD inline int bz_mtf_chunked(const uint8_t *last, int n, const uint8_t *seq_of, int n_in_use, uint16_t *mtfv, uint32_t *freq,
                                int chunks, uint8_t *pos)
{
    uint8_t cur[256], rec[256], tmp[256], yy[256];
    for (int i = 0; i < n_in_use; i++) cur[i] = (uint8_t)i;
    for (int c = 0; c < chunks; c++) {
        const int lo = (int)((long long)n * c / chunks), hi = (int)((long long)n * (c + 1) / chunks);
        const int k = bz_mtf_recency(last, lo, hi, seq_of, rec);
        for (int i = 0; i < n_in_use; i++) yy[i] = cur[i];
        bz_mtf_positions(last, lo, hi, seq_of, yy, pos);
        bz_mtf_combine(cur, rec, k, n_in_use, tmp);
        for (int i = 0; i < n_in_use; i++)
            if (cur[i] != yy[i]) return -1;                     // the combine must give the list the coding ended with
    }
    int w = 0;
    for (int c = 0; c < chunks; c++) {
        const int lo = (int)((long long)n * c / chunks), hi = (int)((long long)n * (c + 1) / chunks);
        w += bz_mtf_code_chunk(pos, lo, hi, n, mtfv + w, freq);
    }
    mtfv[w++] = (uint16_t)(n_in_use + 1); freq[n_in_use + 1]++;
    return w;
}

BZ_HD inline int bz_n_groups(int n_mtf)
{
    return n_mtf < 200 ? 2 : n_mtf < 600 ? 3 : n_mtf < 1200 ? 4 : n_mtf < 2400 ? 5 : 6;
}

// The initial tables: nGroups bands of the alphabet of about equal frequency, each table cheap (0) on its band and dear
// (15) elsewhere, with libbz2's odd-band adjustment.
BZ_HD inline void bz_initial_tables(const uint32_t *freq, int alpha, int n_mtf, int ng, uint8_t (*len)[BZ_MAX_ALPHA])
{
    int n_part = ng, rem = n_mtf, gs = 0;
    while (n_part > 0) {
        int t_freq = rem / n_part, ge = gs - 1, a_freq = 0;
        while (a_freq < t_freq && ge < alpha - 1) { ge++; a_freq += (int)freq[ge]; }
        if (ge > gs && n_part != ng && n_part != 1 && ((ng - n_part) % 2 == 1)) { a_freq -= (int)freq[ge]; ge--; }
        for (int v = 0; v < alpha; v++) len[n_part - 1][v] = (v >= gs && v <= ge) ? 0 : 15;
        n_part--;
        gs = ge + 1;
        rem -= a_freq;
    }
}

// The table that codes group g (symbols [50 g, min(50 g + 50, nMTF))) cheapest; the first one wins a tie.
BZ_HD inline int bz_best_table(const uint16_t *mtfv, int n_mtf, int g, int ng, const uint8_t (*len)[BZ_MAX_ALPHA])
{
    int gs = g * BZ_G_SIZE, ge = gs + BZ_G_SIZE;
    if (ge > n_mtf) ge = n_mtf;
    uint32_t cost[BZ_N_GROUPS] = {0, 0, 0, 0, 0, 0};
    for (int i = gs; i < ge; i++) {
        uint16_t v = mtfv[i];
        for (int t = 0; t < ng; t++) cost[t] += len[t][v];
    }
    int bt = 0;
    for (int t = 1; t < ng; t++)
        if (cost[t] < cost[bt]) bt = t;
    return bt;
}

// BZ2_hbMakeCodeLengths: Huffman code lengths by a binary heap with libbz2's tie-breaks (weights carry the subtree depth
// in their low byte); a code longer than max_len rescales the frequencies (w -> 1 + w / 2) and builds again.
// `work`: BZ_HB_WORK ints of scratch (the kernel passes LDS, one slice per table).
#define BZ_HB_WORK (BZ_MAX_ALPHA + 2 + 4 * BZ_MAX_ALPHA)
BZ_HD inline void bz_make_code_lengths(uint8_t *len, const int32_t *freq, int alpha, int max_len, int32_t *work)
{
    int32_t *heap = work, *weight = work + BZ_MAX_ALPHA + 2, *parent = weight + 2 * BZ_MAX_ALPHA;
    for (int i = 0; i < alpha; i++) weight[i + 1] = (freq[i] == 0 ? 1 : freq[i]) << 8;
    while (true) {
        int n_nodes = alpha, n_heap = 0;
        heap[0] = 0; weight[0] = 0; parent[0] = -2;
        for (int i = 1; i <= alpha; i++) {
            parent[i] = -1;
            n_heap++;
            heap[n_heap] = i;
            int zz = n_heap, tmp = heap[zz];
            while (weight[tmp] < weight[heap[zz >> 1]]) { heap[zz] = heap[zz >> 1]; zz >>= 1; }
            heap[zz] = tmp;
        }
        while (n_heap > 1) {
            int nn[2];
            for (int k = 0; k < 2; k++) {
                nn[k] = heap[1]; heap[1] = heap[n_heap]; n_heap--;
                int zz = 1, tmp = heap[zz];
                while (true) {
                    int yy = zz << 1;
                    if (yy > n_heap) break;
                    if (yy < n_heap && weight[heap[yy + 1]] < weight[heap[yy]]) yy++;
                    if (weight[tmp] < weight[heap[yy]]) break;
                    heap[zz] = heap[yy]; zz = yy;
                }
                heap[zz] = tmp;
            }
            n_nodes++;
            parent[nn[0]] = parent[nn[1]] = n_nodes;
            int32_t w1 = weight[nn[0]], w2 = weight[nn[1]];
            int32_t d1 = w1 & 0xff, d2 = w2 & 0xff;
            weight[n_nodes] = (int32_t)(((uint32_t)w1 & 0xffffff00u) + ((uint32_t)w2 & 0xffffff00u)) | (1 + (d1 > d2 ? d1 : d2));
            parent[n_nodes] = -1;
            n_heap++;
            heap[n_heap] = n_nodes;
            int zz = n_heap, tmp = heap[zz];
            while (weight[tmp] < weight[heap[zz >> 1]]) { heap[zz] = heap[zz >> 1]; zz >>= 1; }
            heap[zz] = tmp;
        }
        bool too_long = false;
        for (int i = 1; i <= alpha; i++) {
            int j = 0, k = i;
            while (parent[k] >= 0) { k = parent[k]; j++; }
            len[i - 1] = (uint8_t)j;
            if (j > max_len) too_long = true;
        }
        if (!too_long) return;
        for (int i = 1; i <= alpha; i++) {
            int j = weight[i] >> 8;
            j = 1 + (j / 2);
            weight[i] = j << 8;
        }
    }
}

// Bits of a block from its final choice: the fixed header, the used map (16 bits per used 16-byte range), the
// MTF-coded selectors in unary, the delta-coded code lengths and the symbols (rfreq of the last pass x final lengths).
BZ_HD inline uint64_t bz_tail_bits(const uint8_t *sel, int n_sel, int ng, const BzTables &tb, int alpha, int used16)
{
    uint64_t bits = BZ_BLOCK_FIXED_BITS + 16u * (uint32_t)used16;
    uint8_t pos[BZ_N_GROUPS];
    for (int i = 0; i < ng; i++) pos[i] = (uint8_t)i;
    for (int i = 0; i < n_sel; i++) {
        uint8_t s = sel[i], tmp = pos[0], tmp2;
        int j = 0;
        while (s != tmp) { j++; tmp2 = tmp; tmp = pos[j]; pos[j] = tmp2; }
        pos[0] = tmp;
        bits += (uint64_t)j + 1;
    }
    for (int t = 0; t < ng; t++) {
        int cur = tb.len[t][0];
        bits += 5;
        for (int v = 0; v < alpha; v++) {
            int d = (int)tb.len[t][v] - cur;
            bits += 1 + 2 * (uint64_t)(d < 0 ? -d : d);
            cur = tb.len[t][v];
            bits += (uint64_t)tb.rfreq[t][v] * tb.len[t][v];
        }
    }
    return bits;
}

// One refinement pass, serially: choose every group's table, count the symbols per chosen table, rebuild the lengths.
BZ_HD inline void bz_refine_serial(const uint16_t *mtfv, int n_mtf, int ng, int alpha, uint8_t *sel, BzTables &tb)
{
    for (int t = 0; t < ng; t++)
        for (int v = 0; v < alpha; v++) tb.rfreq[t][v] = 0;
    const int n_sel = (n_mtf + BZ_G_SIZE - 1) / BZ_G_SIZE;
    for (int g = 0; g < n_sel; g++) {
        int bt = bz_best_table(mtfv, n_mtf, g, ng, tb.len);
        sel[g] = (uint8_t)bt;
        int gs = g * BZ_G_SIZE, ge = gs + BZ_G_SIZE < n_mtf ? gs + BZ_G_SIZE : n_mtf;
        for (int i = gs; i < ge; i++) tb.rfreq[bt][mtfv[i]]++;
    }
    int32_t work[BZ_HB_WORK];
    for (int t = 0; t < ng; t++) bz_make_code_lengths(tb.len[t], tb.rfreq[t], alpha, BZ_MAX_LEN, work);
}

// Bits of one block from its BWT last column, all stages serially (the CPU test's entry; the kernel runs the same
// stages with the chunks and groups spread over a workgroup).  mtfv: room for n + 1 values; sel: room for BZ_MAX_SEL;
// chunks > 0: MTF in that many chunks (pos: n bytes of scratch), else in one pass.  Returns ~0 if the two disagree.
BZ_HD inline uint64_t bz_block_bits_serial(const uint8_t *last, int n, uint16_t *mtfv, uint8_t *sel, BzTables &tb,
                                           int chunks = 0, uint8_t *pos = nullptr)
{
    uint8_t used[256], seq_of[256];
    for (int i = 0; i < 256; i++) used[i] = 0;
    for (int i = 0; i < n; i++) used[last[i]] = 1;
    int n_in_use = 0, used16 = 0;
    for (int i = 0; i < 256; i++)
        if (used[i]) seq_of[i] = (uint8_t)n_in_use++;
    for (int i = 0; i < 16; i++) {
        int u = 0;
        for (int j = 0; j < 16; j++) u |= used[i * 16 + j];
        used16 += u;
    }
    const int alpha = n_in_use + 2;
    uint32_t freq[BZ_MAX_ALPHA];
    for (int i = 0; i < alpha; i++) freq[i] = 0;
    const int n_mtf = chunks > 0 ? bz_mtf_chunked(last, n, seq_of, n_in_use, mtfv, freq, chunks, pos)
                                 : bz_mtf(last, n, seq_of, n_in_use, mtfv, freq);
    if (n_mtf < 0) return ~0ull;
    const int ng = bz_n_groups(n_mtf);
    for (int t = 0; t < BZ_N_GROUPS; t++)
        for (int v = 0; v < alpha; v++) tb.len[t][v] = 15;
    bz_initial_tables(freq, alpha, n_mtf, ng, tb.len);
    for (int it = 0; it < BZ_N_ITERS; it++) bz_refine_serial(mtfv, n_mtf, ng, alpha, sel, tb);
    return bz_tail_bits(sel, (n_mtf + BZ_G_SIZE - 1) / BZ_G_SIZE, ng, tb, alpha, used16);
}
