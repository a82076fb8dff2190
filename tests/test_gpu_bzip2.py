"""GPU parity tests of the bzip2 path: the HIP backend, through the C-ABI and the package,
against the codec the reference calls (the interpreter's bz2.compress).  Bit-exact sizes."""
import bz2
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from snacc_amd import hip_backend
    hip_backend.load()
    return hip_backend


def _acgt(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _mutant(rng, x, rate):
    a = np.frombuffer(x, dtype=np.uint8).copy()
    k = rng.random(a.size) < rate
    a[k] = ACGT[rng.integers(0, 4, int(k.sum()))]
    return a.tobytes()


def _codec_sizes(raw):
    """len(bz2.compress(..)) of every single and ordered pair, on host threads (the call releases the GIL)."""
    n = len(raw)
    with ThreadPoolExecutor() as ex:
        s = list(ex.map(lambda a: len(bz2.compress(a)), raw))
        p = list(ex.map(lambda ij: len(bz2.compress(raw[ij[0]] + raw[ij[1]])), [(i, j) for i in range(n) for j in range(n)]))
    return np.array(s, dtype=np.uint32), np.array(p, dtype=np.uint32).reshape(n, n)


def _check(hip, raw):
    es, ep = _codec_sizes(raw)
    with hip.HipContext(0) as ctx:
        ctx.upload(raw)
        s, p = ctx.bzip2_singles(), ctx.bzip2_pairs()
    assert np.array_equal(s, es), np.flatnonzero(s != es).tolist()
    assert np.array_equal(p, ep), np.argwhere(p != ep)[:8].tolist()
    return s, p


def test_fuzz_ragged_set(hip):
    rng = np.random.default_rng(11)
    lens = [10000, 899981, 899980, 1799962, 2500000, 450000, 123457, 20000, 899990, 1000000, 60000, 333333]
    raw = []
    for k, n in enumerate(lens):
        x = _acgt(rng, n)
        if k % 3 == 1:                         # a run that ends the sequence (continues into y in the pairs)
            x = x[:-300] + b"A" * 300
        if k % 4 == 2:
            x = b"A" * 255 + x[255:]           # a run of 255 at the start: merges with x's final run
        raw.append(x)
    raw += [b"C" * 3 + _acgt(rng, 40000), b"C" + _acgt(rng, 30000) + b"CCC", b"", b"G"]
    _check(hip, raw)


def test_four_1mbp_acgt(hip):
    rng = np.random.default_rng(12)
    _check(hip, [_acgt(rng, 1000000) for _ in range(4)])


def test_two_percent_mutants_of_one_ancestor(hip):
    rng = np.random.default_rng(13)
    anc = _acgt(rng, 1200000)
    _check(hip, [anc] + [_mutant(rng, anc, 0.02) for _ in range(4)])


def test_n_runs_soft_masked_protein_and_periodic(hip):
    rng = np.random.default_rng(14)
    a = bytearray(_acgt(rng, 600000))
    for st in range(1000, len(a) - 5000, 40000):
        a[st:st + 3000] = b"N" * 3000
    b = bytearray(_acgt(rng, 500000))
    b[100000:300000] = bytes(b[100000:300000]).lower()
    prot = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[rng.integers(0, 20, 400000)].tobytes()
    p = 0.5 ** np.arange(20)                                    # a block whose code lengths need the maxLen-17 rescale
    skew = (rng.choice(20, 600000, p=p / p.sum()).astype(np.uint8) + 65)
    skew[rng.integers(0, skew.size, 300)] = rng.integers(128, 256, 300)
    raw = [bytes(a), bytes(b), prot, b"ACGT" * 250000, b"N" * 1000000, bytes(range(256)) * 50, skew.tobytes()]
    _check(hip, raw)


def test_lists_device_rows_and_row_slices_equal_pairs(hip):
    import torch
    rng = np.random.default_rng(15)
    raw = [_acgt(rng, n) for n in (300000, 950000, 70000, 1100000, 5000)]
    with hip.HipContext(0) as ctx:
        ctx.upload(raw)
        full = ctx.bzip2_pairs()
        assert np.array_equal(ctx.bzip2_pairs(1, 4), full[1:4])
        ij = [(i, j) for i in range(5) for j in range(5)][::-1] + [(2, -1)]
        got = ctx.bzip2_pairs_list(ij)
        assert np.array_equal(got[:-1], np.array([full[i, j] for i, j in ij[:-1]], dtype=np.uint32))
        assert got[-1] == ctx.bzip2_singles()[2]
        out = torch.zeros((3, 5), dtype=torch.int32, device="cuda:0")
        ctx.bzip2_pairs_device(2, 5, out.data_ptr(), None)
        ctx.sync(None)
        assert np.array_equal(out.cpu().numpy().astype(np.uint32), full[2:5])
        assert ctx.bzip2_last_ms() > 0
        again = ctx.bzip2_pairs()                    # two runs, identical sizes
        assert np.array_equal(again, full)


def test_all_pairs_and_ncd_matrix(hip):
    from snacc_amd.matrix import ncd_matrix
    from snacc_amd.pairwise_ncd import all_pairs, ncd_matrix_gpu
    rng = np.random.default_rng(16)
    raw = [_acgt(rng, n) for n in (200000, 90000, 400000)]
    singles, pairs = all_pairs(raw, "bzip2")
    es, ep = _codec_sizes(raw)
    assert np.array_equal(singles, es.astype(np.int64) + 33)
    assert np.array_equal(pairs, ep.astype(np.int64) + 33)
    assert np.array_equal(singles, [sys.getsizeof(bz2.compress(a)) for a in raw])
    assert np.array_equal(ncd_matrix_gpu(raw, "bzip2"), ncd_matrix(es.astype(np.int64) + 33, ep.astype(np.int64) + 33))


def _fasta_set(d, rng, k=8):
    from conftest import write_fasta
    d.mkdir(parents=True, exist_ok=True)
    base = _acgt(rng, 150000)
    for i in range(k):
        s = _mutant(rng, base, 0.03) if i % 2 else _acgt(rng, 50000 + 20000 * i)
        write_fasta(d / f"s{i}.fasta", [(f"r{i}", s.decode())])
    return d


@pytest.mark.parametrize("arena_limit", [None, 1000000])
def test_cli_bzip2_csv_equals_thread_pool_flow(hip, tmp_path, monkeypatch, arena_limit):
    from click.testing import CliRunner
    from snacc_amd.cli import cli
    d = _fasta_set(tmp_path / "fa", np.random.default_rng(17))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SNACC_BZIP2", raising=False)
    if arena_limit:
        monkeypatch.setenv("SNACC_ARENA_LIMIT", str(arena_limit))
    a = CliRunner().invoke(cli, [str(d), "-o", "gpu.csv", "-c", "bzip2", "--no-show-progress", "--no-log"])
    monkeypatch.delenv("SNACC_ARENA_LIMIT", raising=False)
    monkeypatch.setenv("SNACC_BZIP2", "stdlib")
    b = CliRunner().invoke(cli, [str(d), "-o", "cpu.csv", "-c", "bzip2", "-n", "8", "--no-show-progress", "--no-log"])
    assert a.exit_code == 0 and b.exit_code == 0, (a.output, b.output)
    assert (tmp_path / "gpu.csv").read_text() == (tmp_path / "cpu.csv").read_text()
