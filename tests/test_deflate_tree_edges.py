"""The oracle's per-block tree facts (oracle/deflate_oracle.c: dfl_oracle_block_lengths, dfl_oracle_block_facts)
and the edge inputs of tests/dfl_edges.py: the facts add up to the stream zlib writes, and every family reaches the
branch of build_tree / flush_block it is meant for.  CPU only; tests/test_gpu_deflate_trees.py runs the same inputs
through the kernel's two tree builders."""
import gzip
import zlib

import numpy as np
import pytest

import dfl_edges as E

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def D():
    from oracle import deflate
    deflate.lib()
    return deflate


def _streams():
    rng = np.random.default_rng(5)
    S = [rng.choice(ACGT, 70000).tobytes(), rng.integers(0, 256, 50000, dtype=np.uint8).tobytes(),
         rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8), 40000).tobytes(),
         np.tile(rng.choice(ACGT, 900), 60).tobytes(), b"", b"A", E.skewed_bytes(40000, 1)]
    S += [b for b, _, _ in E.edge_streams().values()][:12]
    return S


def test_block_facts_add_up_to_the_stream(D):
    """Per block, the facts' bits are the bits trace() reports; the blocks, byte-aligned at the end, are the raw
    stream of gzip.compress / zlib.compress; and the type is the cheapest the facts allow."""
    for x in _streams():
        for level, fn, wrap in ((9, gzip.compress, 18), (6, zlib.compress, 6)):
            r, facts = D.block_facts(x, level=level)
            r2, _, blk = D.trace(x, level=level)
            assert r == r2 == len(fn(x)) - wrap
            assert [int(f["bits"]) for f in facts] == [int(b) for b in blk]
            bits = 0
            for f in facts:
                bits += int(f["bits"])
                opt_b, st_b = (int(f["opt_len"]) + 10) >> 3, (int(f["static_len"]) + 10) >> 3
                best = min(opt_b, st_b)
                if f["type"] == D.STORED:
                    assert f["have_buf"] and int(f["stored_len"]) + 4 <= best
                else:
                    assert int(f["bits"]) == 3 + int(f["static_len"] if f["type"] == D.FIXED else f["opt_len"])
                    assert (f["type"] == D.FIXED) == (st_b <= opt_b)
                assert bool(f["tie"] & D.TIE_STATIC) == (st_b == opt_b)
                assert bool(f["tie"] & D.TIE_STORED) == (int(f["stored_len"]) + 4 == best)
                assert f["tree"][0]["used"] >= 1                          # END_BLOCK
            assert (bits + 7) // 8 == r


def test_block_lengths_prices_like_block_bits(D):
    H = E.histogram_families()
    for name, lf, df in H[::7]:
        f = D.block_lengths(lf, df)
        assert int(f["bits"]) == D.block_bits(lf, df), name
        fixed = (int(f["static_len"]) + 10) >> 3 <= (int(f["opt_len"]) + 10) >> 3
        assert int(f["bits"]) == 3 + int(f["static_len"] if fixed else f["opt_len"]), name


def test_histogram_families_reach_their_branches(D):
    """Each family of the harness histograms reaches its branch on the builder it is meant for.  The overflow count
    of gen_bitlen is always even: it counts the nodes below max_length, and every level of a binary tree below the
    root holds an even number of nodes, so odd counts do not exist."""
    hit = set()
    for name, lf, df in E.histogram_families():
        f = D.block_lengths(lf, df)
        t = f["tree"]
        l2 = lf.copy()
        l2[E.END_BLOCK] = 1
        builder = "lanes" if (l2 > 0).sum() <= 64 else "lds"
        fam = name.split()[0]
        for k, tn in enumerate("LDB"):
            assert t[k]["overflow"] % 2 == 0, name
            if t[k]["overflow"]:
                hit.add((fam, "overflow", tn, builder))
                if fam == "lrepair" and k == 0:
                    hit.add((fam, "overflow", name.split()[3], builder))
        for k in range(t[1]["forced"]):
            hit.add((fam, "forced dist", int(t[1]["forced_code"][k])))
        if t[0]["forced"]:
            hit.add((fam, "forced lit", int(t[0]["forced_code"][0])))
        if fam == "boundary":
            hit.add((fam, int((l2 > 0).sum()), builder))
    need = {("lrepair", "overflow", p, b) for p in ("lit", "len", "mixed") for b in ("lanes", "lds")}
    need |= {("drepair", "overflow", "D", "lanes"), ("blrepair", "overflow", "B", "lanes"), ("blrepair", "overflow", "B", "lds")}
    need |= {("forced", "forced dist", c) for c in (0, 1, 2)} | {("forced", "forced lit", 0)}
    need |= {("boundary", 64, "lanes"), ("boundary", 65, "lds")}
    assert need <= hit, sorted(need - hit)


@pytest.mark.parametrize("name", sorted(E.edge_streams()))
def test_edge_streams_reach_their_branches(D, name):
    """The parser-level inputs (seeds found by search are recorded in tests/dfl_edges.py) still reach their branch, so
    that a generator cannot silently stop covering it."""
    x, level, target = E.edge_streams()[name]
    r, facts = D.block_facts(x, level=level)
    assert E.reaches(facts, target), (name, target)
    fn, wrap = (gzip.compress, 18) if level == 9 else (zlib.compress, 6)
    assert r == len(fn(x)) - wrap
