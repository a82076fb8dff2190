"""The block pricing of the gzip / zlib kernel at its edges (GPU): the two tree builders of
snacc_amd/csrc/snk_deflate.hip.h -- dfl_tree_small on lane arrays, dfl_build_tree on the workgroup's LDS arrays under
G_LOCK -- through the HIP harness tests/hipharness on the histograms of tests/dfl_edges.py, against the oracle's
pricing of the same histograms (zlib 1.2.11's build_tree); and the parser-level edge inputs through the whole path,
against the codec.  Bit-exact."""
import gzip
import zlib

import numpy as np
import pytest

import dfl_edges as E

pytestmark = pytest.mark.gpu

CODEC = {"gzip": gzip.compress, "zlib": zlib.compress}
BATCH = 1024                         # histograms per harness launch: 256 workgroups of four waves


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import hipharness
    hipharness.build()
    return hipharness


@pytest.fixture(scope="module")
def families():
    from oracle import deflate
    H = E.histogram_families()
    facts = [deflate.block_lengths(lf, df) for _, lf, df in H]
    used = [int(((lf > 0) | (np.arange(E.L_CODES) == E.END_BLOCK)).sum()) for _, lf, _ in H]
    order = E.lock_contention_order(H, [u > 64 for u in used])
    assert sorted(order) == list(range(len(H)))
    H = [H[i] for i in order]
    return (H, np.array([int(facts[i]["opt_len"]) for i in order]), np.array([int(facts[i]["static_len"]) for i in order]),
            np.array([used[i] > 64 for i in order]))


def _run(harness, H, mode):
    hist = np.stack([np.concatenate([lf, df]) for _, lf, df in H])
    parts = [harness.run(hist[i:i + BATCH], mode) for i in range(0, len(hist), BATCH)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _check(H, got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, len(bad), [(H[i][0], int(got[i]), int(want[i])) for i in bad[:6]])


def test_tree_builders_price_like_zlib(harness, families):
    """As dfl_flush_body chooses (lane arrays up to 64 used symbols, else the LDS builder under the lock; the first
    workgroups have all four waves on the LDS builder at once, the next ones mix both): opt_len and static_len of
    every histogram equal the oracle's -- the length-limit repair of all three trees, forced codes, ties, the
    64 / 65 boundary, the largest block and random blocks."""
    H, opt, st, big = families
    o, s, lds = _run(harness, H, 0)
    assert np.array_equal(lds.astype(bool), big), "builder choice"
    _check(H, o, opt, "opt_len")
    _check(H, s, st, "static_len")


def test_lds_builder_prices_every_histogram_like_zlib(harness, families):
    """The LDS builder on every histogram, the small alphabets too, four waves of a workgroup taking turns on it."""
    H, opt, st, _ = families
    o, s, lds = _run(harness, H, 1)
    assert lds.all()
    _check(H, o, opt, "opt_len")
    _check(H, s, st, "static_len")


def _edge_set():
    """The parser-level edge inputs (each once), shorter relatives of them, and 16 byte-alphabet sequences so that
    many waves of one launch take the LDS builder."""
    seen, seqs = set(), []
    for x, _, _ in E.edge_streams().values():
        if x not in seen:
            seen.add(x)
            seqs.append(x)
    rel = [x[: len(x) // 2] + x[-len(x) // 3:] for x in seqs if len(x) > 1000]
    rng = np.random.default_rng(404)
    byteset = [E.skewed_bytes(int(rng.integers(3000, 20000)), 100 + i, spread=float(rng.uniform(4, 13))) for i in range(16)]
    return seqs + rel + byteset


@pytest.fixture(scope="module")
def edge_expect():
    seqs = _edge_set()
    exp = {}
    for alg, fn in CODEC.items():
        exp[alg] = (np.array([len(fn(a)) for a in seqs], dtype=np.uint32),
                    np.array([[len(fn(a + b)) for b in seqs] for a in seqs], dtype=np.uint32))
    return seqs, exp


@pytest.mark.parametrize("options", [{}, {"deflate_serial": 1}, {"deflate_kmer": 0}, {"deflate_norestart": 1}],
                         ids=["default", "serial", "nokmer", "norestart"])
def test_edge_streams_through_the_kernels(edge_expect, options):
    """Singles and every ordered pair of the edge inputs -- bit-length repair, forced codes, ties, stored blocks,
    big alphabets, each in x before the restart point, across the seam and in y -- against gzip / zlib."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from snacc_amd import hip_backend
    hip_backend.load()
    seqs, exp = edge_expect
    with hip_backend.HipContext(0, **options) as ctx:
        ctx.upload([np.frombuffer(x, dtype=np.uint8) for x in seqs])
        for alg in CODEC:
            s, p = ctx.deflate_singles(alg), ctx.deflate_pairs(alg)
            es, ep = exp[alg]
            assert np.array_equal(s, es), (alg, options, np.flatnonzero(s != es))
            assert np.array_equal(p, ep), (alg, options, np.argwhere(p != ep)[:5])
