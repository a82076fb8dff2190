"""Inputs that drive the deflate block pricing into its rare branches (TEST INFRASTRUCTURE): zlib's build_tree +
gen_bitlen as the gzip / zlib kernel restates it twice (dfl_tree_small on lane arrays, dfl_build_tree on the
workgroup's LDS arrays; snacc_amd/csrc/snk_deflate.hip.h).

* ``histogram_families()`` -- block histograms (286 literal/length + 30 distance counts) for the HIP harness
  tests/hipharness: the length-limit repair of each tree, forced codes, count ties, the 64 / 65 used-symbol
  boundary between the two builders, the largest block, random blocks.
* ``edge_streams()`` -- byte strings whose zlib parse (level 9 for gzip, 6 for zlib) closes blocks that reach the
  same branches through the real parser.

Everything is deterministic; the seeds found by search are recorded here.  Which branch an input reaches is
checked against the oracle (oracle.deflate.block_lengths / block_facts) by tests/test_deflate_tree_edges.py."""
import functools

import numpy as np

L_CODES, D_CODES, END_BLOCK = 286, 30, 256
BLOCK = 16383            # symbols per block (zlib's lit_bufsize - 1)
MAX_DIST = 32506         # farthest match zlib takes (w_size - MIN_LOOKAHEAD)
LENGTH_CODES = np.arange(257, 286)

# Seeds of bit-length trees deeper than 7 bits (the 7-bit repair), found by search against the oracle's overflow
# count with _geometric_hist: (seed, used-symbol limit).  64: the lane-array builder takes the block, 286: the LDS one.
BL_REPAIR_SEEDS = [(1915, 64), (2425, 64), (3078, 64), (3243, 64), (3602, 64),
                   (3, 286), (17, 286), (29, 286), (87, 286), (126, 286)]


def fib(k, a=1, b=1):
    out = []
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return np.array(out, dtype=np.int64)


def _empty():
    return np.zeros(L_CODES, np.int64), np.zeros(D_CODES, np.int64)


def _geometric_hist(seed, max_used):
    """Counts spread over many powers of two: code lengths of many different values with skewed frequencies,
    i.e. a skewed bit-length alphabet of 9 or more symbols."""
    rng = np.random.default_rng(seed)
    lf, df = _empty()
    k = int(rng.integers(20, min(max_used, 200)))
    pos = rng.choice(L_CODES, k, replace=False)
    lf[pos] = np.maximum(1, (2.0 ** rng.uniform(0, rng.uniform(6, 13), k)).astype(np.int64))
    kd = int(rng.integers(0, 30))
    if kd:
        df[rng.choice(D_CODES, kd, replace=False)] = np.maximum(1, (2.0 ** rng.uniform(0, 10, kd)).astype(np.int64))
    return lf, df


def _fib_counts(k, variant, end_block=False):
    """k Fibonacci-like counts, sum < 2^16 (the builders keep node counts in 16 bits; a real block holds at most
    16 383 symbols).  Fibonacci counts are the cheapest way to a deep tree, a chain of depth k - 1 for the sum
    F(k + 2) - 1, so 16 bits allow depth 22 at most.  end_block: the literal/length tree has END_BLOCK (count 1)
    too, which takes the place of the first 1 (another 1 would pair the leaves up and halve the depth).
    Longer sequences start with a run of ones (a balanced subtree at the bottom).  variant 1 starts 1, 2, 3, 5;
    variant 2 puts two more ones below the chain."""
    a, b, extra = ((1, 1, 0), (1, 2, 0), (1, 1, 2))[variant]
    chain = fib(k + 1, a, b)[1:] if end_block and variant != 1 else fib(k, a, b)
    cap = 21 if variant != 1 else 20
    if k > cap:
        chain = np.concatenate([np.ones(k - cap, np.int64), chain[:cap]])
    if extra:
        chain = np.concatenate([np.ones(extra, np.int64), chain[:k - extra]])
    return chain


def histogram_families():
    """[(name, lfreq[286], dfreq[30])] -- END_BLOCK is forced to 1 by the harness and the oracle alike."""
    H = []
    rng = np.random.default_rng(2024)
    lit_pool = np.array([c for c in range(256)], dtype=np.int64)
    # literal/length repair: Fibonacci counts on literals, on length codes (extra bits), mixed; both builders
    for k in range(17, 31):
        for variant in (0, 1, 2):
            counts = _fib_counts(k, variant, end_block=True)
            for place in ("lit", "len", "mixed"):
                if place == "len" and k > 29:
                    continue
                if place == "lit":
                    pos = rng.choice(lit_pool, k, replace=False)
                elif place == "len":
                    pos = rng.choice(LENGTH_CODES, k, replace=False)
                else:
                    pos = rng.choice(np.concatenate([lit_pool, LENGTH_CODES]), k, replace=False)
                for big in (False, True):
                    lf, df = _empty()
                    lf[pos] = counts[rng.permutation(k)]
                    free = np.setdiff1d(np.arange(L_CODES), np.append(pos, END_BLOCK))
                    # filler: a few heavy symbols on top (deepens the chain), up to 64 used, or 65 and more
                    nfill = int(rng.integers(66 - k, 120 - k)) if big else int(rng.integers(1, 64 - k))
                    fill = rng.choice(free, nfill, replace=False)
                    budget = (1 << 16) - 1 - int(lf.sum()) - 64
                    lf[fill] = np.maximum(1, budget // max(1, nfill) // int(rng.integers(1, 4)))
                    df[rng.choice(D_CODES, 3, replace=False)] = rng.integers(1, 20, 3)
                    H.append((f"lrepair k={k} v={variant} {place} {'lds' if big else 'lanes'}", lf, df))
    # distance repair: Fibonacci counts over 17..30 distance codes
    for k in range(17, 31):
        for variant in (0, 1):
            lf, df = _empty()
            df[rng.choice(D_CODES, k, replace=False)] = _fib_counts(k, variant)[rng.permutation(k)]
            lf[rng.choice(LENGTH_CODES, 10, replace=False)] = rng.integers(1, 500, 10)
            lf[rng.choice(lit_pool, 20, replace=False)] = rng.integers(1, 500, 20)
            H.append((f"drepair k={k} v={variant}", lf, df))
    # bit-length repair (7 bits)
    for seed, limit in BL_REPAIR_SEEDS:
        lf, df = _geometric_hist(seed, limit)
        H.append((f"blrepair seed={seed}", lf, df))
    # forced codes
    for lits in ([], [0], [1], [255], [65, 66]):
        for dists in ([], [0], [1], [2], [29], [0, 1]):
            lf, df = _empty()
            lf[lits] = 7
            df[dists] = 3
            if dists:
                lf[257] = 3 * len(dists)
            H.append((f"forced lits={lits} dists={dists}", lf, df))
    # ties: all counts equal, and powers of two
    for n in list(range(2, 65)) + [65, 66, 80, 100, 128, 129, 200, 255, 256, 285]:
        for c in (1, 3, 64):
            lf, df = _empty()
            pos = np.setdiff1d(np.arange(L_CODES), [END_BLOCK])[:n] if n < 150 else rng.choice(
                np.setdiff1d(np.arange(L_CODES), [END_BLOCK]), n, replace=False)
            lf[pos] = c
            df[: min(n, 30)] = c
            H.append((f"equal n={n} c={c}", lf, df))
    for n in (8, 16, 30, 64, 100):
        lf, df = _empty()
        pos = rng.choice(np.setdiff1d(np.arange(L_CODES), [END_BLOCK]), n, replace=False)
        lf[pos] = 2 ** (np.arange(n) % 12)
        df[:] = 2 ** (np.arange(30) % 10)
        H.append((f"pow2 n={n}", lf, df))
    # the 64 / 65 boundary (END_BLOCK included in the count), END_BLOCK first / in the middle / last of the used codes
    for used in (63, 64, 65, 66):
        for where in ("last", "middle", "first"):
            others = used - 1
            if where == "last":
                pos = np.arange(256 - others, 256)
            elif where == "middle":
                nlen = min(others // 2, 29)
                pos = np.concatenate([np.arange(256 - (others - nlen), 256), np.arange(257, 257 + nlen)])
            else:
                pos = np.arange(257, 257 + min(others, 29))
                pos = np.concatenate([pos, np.arange(others - len(pos))])
            lf, df = _empty()
            lf[pos] = rng.integers(1, 300, len(pos))
            df[rng.choice(D_CODES, 5, replace=False)] = rng.integers(1, 50, 5)
            H.append((f"boundary used={used} end_block {where}", lf, df))
    # the largest block: one symbol 16 382 times, the rest once
    for rest in (1, 3, 40, 63, 64, 120, 285):
        for big in (65, 0, 285):
            lf, df = _empty()
            lf[big] = 16382
            others = np.setdiff1d(np.arange(L_CODES), [big, END_BLOCK])[:rest]
            lf[others] = 1
            df[: min(rest, 30)] = 1
            H.append((f"largest sym={big} rest={rest}", lf, df))
    # random blocks of DNA, protein and byte shape
    for i in range(1500):
        lf, df = _empty()
        shape = i % 3
        lits = rng.choice(256, (4, 20, int(rng.integers(30, 256)))[shape], replace=False)
        lf[lits] = rng.integers(1, (3000, 600, 80)[shape], len(lits))
        nl = int(rng.integers(0, 29))
        lf[rng.choice(LENGTH_CODES, nl, replace=False)] = rng.integers(1, 400, nl)
        nd = int(rng.integers(0, 31))
        df[rng.choice(D_CODES, nd, replace=False)] = rng.integers(1, 400, nd)
        H.append((f"random {('dna', 'protein', 'bytes')[shape]} {i}", lf, df))
    for name, lf, df in H:
        assert lf.sum() + df.sum() + 1 < 1 << 16, name
    return H


def lock_contention_order(H, used_big):
    """Indices of H ordered so that the first workgroups (4 waves each) hold only LDS-builder histograms and the ones
    after them mix both builders, one LDS histogram per workgroup next to three lane-array ones."""
    big = [i for i in range(len(H)) if used_big[i]]
    small = [i for i in range(len(H)) if not used_big[i]]
    nbig_groups = len(big) // 2 // 4
    order = big[: 4 * nbig_groups]
    rest_big, k = big[4 * nbig_groups:], 0
    for b in rest_big:
        order.append(b)
        order.extend(small[k:k + 3])
        k += 3
    order.extend(small[k:])
    return order


# ---------------------------------------------------------------------------------------------------------------
# byte streams through the real parser
# ---------------------------------------------------------------------------------------------------------------

# Random inputs whose single block is decided by a tie, found by search against the oracle's facts:
# (seed, length, letters from 'A' on, level).  _tie_input builds them.
STATIC_TIE_SEEDS = [(947, 17, 9), (1827, 2, 9)]          # static_lenb == dynamic opt_lenb: fixed Huffman
STORED_TIE_SEEDS = [21, 24, 31, 36]                       # random bytes: stored_len + 4 == opt_lenb, stored


def _static_tie_input(seed, letters):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 3000))
    rng.integers(2, 40)
    return bytes(rng.choice(np.arange(65, 65 + letters), n).astype(np.uint8))


def _stored_tie_input(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 120))
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def fresh_background(n, alphabet, seed):
    """n bytes over `alphabet` in which no three-byte string occurs twice (while the alphabet allows it): nothing in
    it matches, so every match of a stream built on it is a planted one."""
    rng = np.random.default_rng(seed)
    alphabet = np.asarray(alphabet, dtype=np.int64)
    seen = np.zeros((256, 256, 256), dtype=bool)
    out = np.empty(n, dtype=np.uint8)
    out[:2] = rng.choice(alphabet, 2)
    for i in range(2, n):
        a, b = out[i - 2], out[i - 1]
        cand = alphabet[~seen[a, b, alphabet]]
        c = int(rng.choice(cand)) if len(cand) else int(rng.choice(alphabet))
        seen[a, b, c] = True
        out[i] = c
    return out


def one_match_stream(dist, seed, n=400):
    """Fresh bytes with exactly one match, 6 bytes at `dist`: a distance tree of one code (zlib forces a second)."""
    bg = fresh_background(max(n, dist + 300), np.arange(256), seed)
    p = len(bg) - 100
    out = bytearray(bg)
    for i in range(p, p + 6):                     # byte by byte: a run when dist < 6
        out[i] = out[i - dist]
    out[p + 6] = (out[p + 6 - dist] + 1) % 256
    return bytes(out)


def skewed_bytes(n, seed, spread=13.0):
    """Bytes with frequencies spread over many powers of two: code lengths of many values with skewed counts, whose
    bit-length tree needs more than 7 bits."""
    rng = np.random.default_rng(seed)
    p = 2.0 ** -rng.uniform(0, spread, 256)
    return bytes(rng.choice(256, n, p=p / p.sum()).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def edge_streams():
    """{name: (bytes, level, target)}: inputs whose zlib parse at `level` (9: gzip, 6: zlib) reaches `target` in at
    least one block -- checked by tests/test_deflate_tree_edges.py.  Targets: 'bl_repair' (bit-length tree over 7
    bits), 'forced_dist=<codes>' (forced distance codes), 'forced_lit' (END_BLOCK alone), 'end_plus_one' (END_BLOCK
    and one literal), 'static_tie', 'stored_tie', 'lds' (a block of more than 64 literal/length symbols).

    Not reached through the parser: the 15-bit repair of the literal/length and distance trees.  A block holds
    16 383 symbols, so planted copies with Fibonacci counts fit for about 17 codes, one chain level short of 15
    bits at the bottom; and chance matches at the literal that breaks each copy add rare codes that pair up the
    bottom of the chain and take the depth away.  The harness histograms (histogram_families) cover both repairs."""
    E = {}
    for lv in (9, 6):
        for seed in (1, 2, 5):
            E[f"skewed s={seed} l={lv}"] = (skewed_bytes(40000, seed), lv, "bl_repair")
        for dist, forced in ((1, "1"), (2, "2"), (5, "0"), (25000, "0")):
            E[f"one match d={dist} l={lv}"] = (one_match_stream(dist, dist), lv, "forced_dist=" + forced)
        E[f"empty l={lv}"] = (b"", lv, "forced_lit")
        for c in (0, 1, 255):
            E[f"byte {c} l={lv}"] = (bytes([c]), lv, "end_plus_one")
        for seed in STORED_TIE_SEEDS:
            E[f"stored tie s={seed} l={lv}"] = (_stored_tie_input(seed), lv, "stored_tie")
        E[f"random bytes l={lv}"] = (fresh_background(30000, np.arange(256), 77).tobytes(), lv, "lds")
    for seed, letters, lv in STATIC_TIE_SEEDS:
        E[f"static tie s={seed} l={lv}"] = (_static_tie_input(seed, letters), lv, "static_tie")
    return E


def reaches(facts, target):
    """Does one of the blocks (oracle.deflate.block_facts) reach `target`?"""
    for f in facts:
        t = f["tree"]
        if target == "bl_repair" and t[2]["overflow"] > 0:
            return True
        if target.startswith("forced_dist=") and t[1]["forced"] > 0 and \
                ",".join(str(int(c)) for c in t[1]["forced_code"][:t[1]["forced"]]) == target[12:]:
            return True
        if target == "forced_lit" and t[0]["forced"] == 1 and t[0]["used"] == 1:
            return True
        if target == "end_plus_one" and t[0]["used"] == 2 and t[0]["forced"] == 0:
            return True
        if target == "static_tie" and f["tie"] & 1 and f["type"] == 1:
            return True
        if target == "stored_tie" and f["tie"] & 2 and f["have_buf"] and f["type"] == 0:
            return True
        if target == "lds" and t[0]["used"] > 64:
            return True
    return False
