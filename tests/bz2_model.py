"""A CPU model of the bzip2 codec at level 9 (what ``bz2.compress`` writes), stage by stage, independent of the
HIP sources: RLE1 and the block cut, the BWT (cyclic rotations, prefix doubling with numpy), MTF with the
RUNA/RUNB zero-run coding, the table choice and code lengths of ``sendMTFValues``, and the bit stream.

:func:`compress` emits real bytes; for every input whose blocks have no tied rotations they equal
``bz2.compress`` byte for byte (tied rotations only move ``origPtr`` inside its fixed 24 bits, so the size
is the same).  :func:`block_bits` and :func:`stream_size` give the bit count of a block and the size of a
stream without writing bytes; :func:`pair_size` composes ``len(bz2.compress(x + y))`` from x's kept block
bits and the blocks recomputed for the pair."""
import zlib

import numpy as np

LEVEL = 9
NBLOCK_MAX = 100000 * LEVEL - 19          # a block is cut once it holds this many RLE1 bytes
N_ITERS = 4
G_SIZE = 50
MAX_LEN = 17
_REV8 = bytes(int(f"{b:08b}"[::-1], 2) for b in range(256))


def crc32_msb(data):
    """bzip2's CRC (CRC-32/BZIP2: polynomial 0x04c11db7, MSB first): the bit-reversed zlib CRC of bit-reversed bytes."""
    c = zlib.crc32(bytes(data).translate(_REV8))
    return int(f"{c:032b}"[::-1], 2)


# ---- RLE1 and the block cut ---------------------------------------------------------------------------------------
def rle1_units(data, start=0):
    """The RLE1 units of data[start:] in order: (raw_begin, raw_end, emitted bytes).  A run of 1-3 bytes is itself,
    a run of 4-255 is 4 bytes plus a count byte (length - 4); longer runs are cut every 255 bytes."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)[start:]
    n = a.size
    if n == 0:
        return []
    change = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.concatenate(([0], change))
    ends = np.concatenate((change, [n]))
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        ch = int(a[s])
        while s < e:
            k = min(255, e - s)
            out.append((start + s, start + s + k, bytes([ch]) * k if k < 4 else bytes([ch] * 4 + [k - 4])))
            s += k
    return out


def blocks(data, start=0):
    """The blocks of data[start:] as lists of RLE1 units: a block is cut after the unit that brings it to
    NBLOCK_MAX bytes or more; the last unit (the run pending at the end of the input) joins the last block."""
    out, cur, nb = [], [], 0
    for u in rle1_units(data, start):
        cur.append(u)
        nb += len(u[2])
        if nb >= NBLOCK_MAX:
            out.append(cur)
            cur, nb = [], 0
    if cur:
        out.append(cur)
    return out


# ---- BWT --------------------------------------------------------------------------------------------------------------
def bwt(block):
    """(last column, origPtr) of the sorted cyclic rotations of `block` (bytes), by prefix doubling."""
    b = np.frombuffer(block, dtype=np.uint8).astype(np.int64)
    n = b.size
    rank = b.copy()
    h = 1
    while True:
        second = rank[(np.arange(n) + h) % n]
        order = np.lexsort((second, rank))
        k1, k2 = rank[order], second[order]
        head = np.ones(n, dtype=bool)
        head[1:] = (k1[1:] != k1[:-1]) | (k2[1:] != k2[:-1])
        new = np.empty(n, dtype=np.int64)
        new[order] = np.cumsum(head) - 1
        rank = new
        if head.all() or h >= n:
            break
        h *= 2
    order = np.argsort(rank, kind="stable")
    last = b[(order - 1) % n].astype(np.uint8)
    return last.tobytes(), int(np.flatnonzero(order == 0)[0])


# ---- MTF and the zero-run coding -------------------------------------------------------------------------------------
def mtf(last, in_use):
    """mtfv (RUNA = 0, RUNB = 1, MTF position j -> j + 1, EOB = nInUse + 1) of a BWT last column."""
    seq_of = {c: i for i, c in enumerate(in_use)}
    n_in_use = len(in_use)
    yy = list(range(n_in_use))
    out = []
    z = 0

    def flush(z):
        z -= 1
        while True:
            out.append(1 if z & 1 else 0)
            if z < 2:
                break
            z = (z - 2) // 2

    for c in last:
        s = seq_of[c]
        if yy[0] == s:
            z += 1
            continue
        if z:
            flush(z)
            z = 0
        j = yy.index(s)
        del yy[j]
        yy.insert(0, s)
        out.append(j + 1)
    if z:
        flush(z)
    out.append(n_in_use + 1)
    return np.array(out, dtype=np.int64)


# ---- Huffman code lengths (BZ2_hbMakeCodeLengths) --------------------------------------------------------------------
def make_code_lengths(freq, max_len=MAX_LEN):
    alpha = len(freq)
    weight = [0] * (2 * alpha + 2)
    for i in range(alpha):
        weight[i + 1] = (freq[i] if freq[i] else 1) << 8
    while True:
        n_nodes, n_heap = alpha, 0
        heap = [0] * (alpha + 2)
        parent = [-1] * (2 * alpha + 2)
        weight[0] = 0
        parent[0] = -2

        def up(z):
            tmp = heap[z]
            while weight[tmp] < weight[heap[z >> 1]]:
                heap[z] = heap[z >> 1]
                z >>= 1
            heap[z] = tmp

        def down(z):
            tmp = heap[z]
            while True:
                y = z << 1
                if y > n_heap:
                    break
                if y < n_heap and weight[heap[y + 1]] < weight[heap[y]]:
                    y += 1
                if weight[tmp] < weight[heap[y]]:
                    break
                heap[z] = heap[y]
                z = y
            heap[z] = tmp

        for i in range(1, alpha + 1):
            n_heap += 1
            heap[n_heap] = i
            up(n_heap)
        while n_heap > 1:
            n1 = heap[1]; heap[1] = heap[n_heap]; n_heap -= 1; down(1)                      # noqa: E702
            n2 = heap[1]; heap[1] = heap[n_heap]; n_heap -= 1; down(1)                      # noqa: E702
            n_nodes += 1
            parent[n1] = parent[n2] = n_nodes
            w1, w2 = weight[n1], weight[n2]
            weight[n_nodes] = ((w1 & 0xFFFFFF00) + (w2 & 0xFFFFFF00)) | (1 + max(w1 & 0xFF, w2 & 0xFF))
            parent[n_nodes] = -1
            n_heap += 1
            heap[n_heap] = n_nodes
            up(n_heap)
        lens, too_long = [], False
        for i in range(1, alpha + 1):
            j, k = 0, i
            while parent[k] >= 0:
                k = parent[k]
                j += 1
            lens.append(j)
            too_long |= j > max_len
        if not too_long:
            return lens
        for i in range(1, alpha + 1):
            weight[i] = (1 + ((weight[i] >> 8) // 2)) << 8


# ---- table choice (sendMTFValues) ---------------------------------------------------------------------------------
def n_groups(n_mtf):
    return 2 if n_mtf < 200 else 3 if n_mtf < 600 else 4 if n_mtf < 1200 else 5 if n_mtf < 2400 else 6


def choose_tables(mtfv, alpha):
    """(nGroups, code lengths [nGroups][alpha], selectors, rfreq of the last iteration) as libbz2 1.0.8 chooses them."""
    n_mtf = mtfv.size
    freq = np.bincount(mtfv, minlength=alpha)
    ng = n_groups(n_mtf)
    lens = np.full((6, alpha), 15, dtype=np.int64)
    n_part, rem, gs = ng, n_mtf, 0
    while n_part > 0:
        t_freq = rem // n_part
        ge, a_freq = gs - 1, 0
        while a_freq < t_freq and ge < alpha - 1:
            ge += 1
            a_freq += int(freq[ge])
        if ge > gs and n_part != ng and n_part != 1 and (ng - n_part) % 2 == 1:
            a_freq -= int(freq[ge])
            ge -= 1
        lens[n_part - 1, :] = 15
        lens[n_part - 1, gs:ge + 1] = 0
        n_part -= 1
        gs = ge + 1
        rem -= a_freq
    lens = lens[:ng]
    n_sel = (n_mtf + G_SIZE - 1) // G_SIZE
    group = np.arange(n_mtf) // G_SIZE
    for _ in range(N_ITERS):
        cost = np.zeros((ng, n_sel), dtype=np.int64)
        for t in range(ng):
            cost[t] = np.bincount(group, weights=lens[t][mtfv], minlength=n_sel).astype(np.int64)
        sel = np.argmin(cost, axis=0)                                         # first table wins ties
        rfreq = np.zeros((ng, alpha), dtype=np.int64)
        np.add.at(rfreq, (sel[group], mtfv), 1)
        lens = np.array([make_code_lengths(rfreq[t].tolist()) for t in range(ng)], dtype=np.int64)
    return ng, lens, sel, rfreq


def selector_mtf(sel, ng):
    pos = list(range(ng))
    out = []
    for s in sel.tolist():
        j = pos.index(s)
        del pos[j]
        pos.insert(0, s)
        out.append(j)
    return out


def _block_parts(block):
    """Everything a block's bits depend on: (in_use, ng, lens, sel, rfreq, mtfv, last, origPtr)."""
    last, orig = bwt(block)
    in_use = sorted(set(block))
    mtfv = mtf(last, in_use)
    ng, lens, sel, rfreq = choose_tables(mtfv, len(in_use) + 2)
    return in_use, ng, lens, sel, rfreq, mtfv, last, orig


def block_bits(block):
    """Bits of one compressed block (header through the last symbol): the size model the kernels restate."""
    in_use, ng, lens, sel, rfreq, mtfv, _, _ = _block_parts(block)
    used16 = len({c >> 4 for c in in_use})
    bits = 48 + 32 + 1 + 24 + 16 + 16 * used16 + 3 + 15
    bits += sum(j + 1 for j in selector_mtf(sel, ng))
    for t in range(ng):
        prev = int(lens[t][0])
        bits += 5
        for v in lens[t].tolist():
            bits += 1 + 2 * abs(v - prev)
            prev = v
    bits += int((rfreq * lens).sum())
    return bits


def stream_size(block_bit_counts):
    """len(bz2.compress(...)) from the bits of its blocks: 'BZh9', the blocks, end-of-stream marker and CRC, padding."""
    return 4 + (sum(block_bit_counts) + 80 + 7) // 8


def block_bytes(blk):
    return b"".join(u[2] for u in blk)


def size(data):
    return stream_size([block_bits(block_bytes(b)) for b in blocks(data)])


def pair_size(x, y, x_block_bits=None):
    """len(bz2.compress(x + y)) from x's blocks before its last one (kept) plus the blocks of x + y from the first
    raw byte of x's last block on (recomputed)."""
    bx = blocks(x)
    kept = bx[:-1]
    start = bx[-1][0][0] if bx else 0
    if x_block_bits is None:
        x_block_bits = [block_bits(block_bytes(b)) for b in kept]
    new = [block_bits(block_bytes(b)) for b in blocks(bytes(x) + bytes(y), start)]
    return stream_size(list(x_block_bits[:len(kept)]) + new)


# ---- the bit stream ----------------------------------------------------------------------------------------------
def compress(data):
    """The bytes of bz2.compress(data) (level 9)."""
    out = ["".join(f"{c:08b}" for c in b"BZh9")]
    w = out.append
    combined = 0
    for blk in blocks(data):
        raw_crc = crc32_msb(b"".join(bytes([u[2][0]]) * (u[1] - u[0]) for u in blk))
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ raw_crc
        block = block_bytes(blk)
        in_use, ng, lens, sel, rfreq, mtfv, last, orig = _block_parts(block)
        for c in b"\x31\x41\x59\x26\x53\x59":
            w(f"{c:08b}")
        w(f"{raw_crc:032b}")
        w("0")
        w(f"{orig:024b}")
        used = set(in_use)
        used16 = [any(16 * i + j in used for j in range(16)) for i in range(16)]
        w("".join("1" if u else "0" for u in used16))
        for i in range(16):
            if used16[i]:
                w("".join("1" if 16 * i + j in used else "0" for j in range(16)))
        w(f"{ng:03b}")
        w(f"{sel.size:015b}")
        w("".join("1" * j + "0" for j in selector_mtf(sel, ng)))
        codes = []
        for t in range(ng):
            ln = lens[t].tolist()
            code, vec = [0] * len(ln), 0
            for n in range(min(ln), max(ln) + 1):
                for i, v in enumerate(ln):
                    if v == n:
                        code[i] = vec
                        vec += 1
                vec <<= 1
            codes.append([f"{c:0{v}b}" for c, v in zip(code, ln)])
            cur = ln[0]
            w(f"{cur:05b}")
            for v in ln:
                w(("10" * (v - cur) if v > cur else "11" * (cur - v)) + "0")
                cur = v
        group_sel = sel[np.arange(mtfv.size) // G_SIZE].tolist()
        w("".join(codes[t][v] for t, v in zip(group_sel, mtfv.tolist())))
    for c in b"\x17\x72\x45\x38\x50\x90":
        w(f"{c:08b}")
    w(f"{combined:032b}")
    s = "".join(out)
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big")
