"""CLI routing of ``-c bzip2`` without a GPU: a context whose sizes come from ``bz2.compress`` (the ctx_factory hook of
cli.gpu_matrix) stands in for the HIP backend.  The GPU route writes the CSV the reference's thread-pool flow writes
(SNACC_BZIP2=stdlib), also through the blocked path (SNACC_ARENA_LIMIT); ``-s`` keeps the thread-pool flow."""
import bz2

import numpy as np
import pytest
from click.testing import CliRunner

from conftest import write_fasta


class _Bz2Context:
    """Stands in for HipContext: bzip2 sizes (no getsizeof overhead) from the interpreter's codec."""
    arena_limit = None

    def __init__(self, device):
        self.device = device
        self.seqs = []
        self.options = {}
        self.calls = []

    def set_option(self, key, value):
        self.options[key] = value

    def upload_fasta(self, paths, reverse_complement=False):
        from snacc_amd import fasta
        from snacc_amd.hip_backend import ArenaTooBig
        seqs = [fasta.read_sequence(p, reverse_complement).encode() for p in paths]
        if self.arena_limit is not None and sum(len(s) + 128 for s in seqs) >= self.arena_limit:
            raise ArenaTooBig("ASCII arena exceeds the offset range of one upload")
        self.seqs = seqs
        self.n = len(seqs)

    def lengths(self):
        return np.array([len(s) for s in self.seqs], dtype=np.uint64)

    def bzip2_singles(self):
        self.calls.append("singles")
        return np.array([len(bz2.compress(s)) for s in self.seqs], dtype=np.uint32)

    def bzip2_pairs(self, r0=0, r1=None):
        self.calls.append("pairs")
        r1 = self.n if r1 is None else r1
        return np.array([[len(bz2.compress(self.seqs[i] + b)) for b in self.seqs] for i in range(r0, r1)], dtype=np.uint32)

    def bzip2_pairs_list(self, ij):
        self.calls.append("pairs_list")
        return np.array([len(bz2.compress(self.seqs[i] + (self.seqs[j] if j >= 0 else b""))) for i, j in ij], dtype=np.uint32)

    def close(self):
        pass


def _fasta_dir(d, k=5):
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    d.mkdir()
    base = acgt[rng.integers(0, 4, 6000)].tobytes()
    for i in range(k):
        s = base[: 3000 + 500 * i] + acgt[rng.integers(0, 4, 2000 + 700 * i)].tobytes() + b"N" * (40 * i)
        write_fasta(d / f"g{i}.fasta", [(f"r{i}", s.decode())])
    return d


@pytest.fixture
def routed(monkeypatch):
    """cli.gpu_matrix with the bz2-backed context; records the contexts it made."""
    from snacc_amd import cli as cli_mod
    made = []

    def factory(dev):
        made.append(_Bz2Context(dev))
        made[-1].arena_limit = int(__import__("os").environ["SNACC_ARENA_LIMIT"]) if "SNACC_ARENA_LIMIT" in __import__("os").environ else None
        return made[-1]

    real = cli_mod.gpu_matrix
    monkeypatch.setattr(cli_mod, "gpu_matrix", lambda *a, **k: real(*a, ctx_factory=factory, **k))
    return cli_mod, made


@pytest.mark.parametrize("arena_limit", [None, 30000])
def test_bzip2_gpu_route_writes_the_thread_pool_csv(tmp_path, monkeypatch, routed, arena_limit):
    cli_mod, made = routed
    d = _fasta_dir(tmp_path / "fa")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SNACC_BZIP2", raising=False)
    if arena_limit:
        monkeypatch.setenv("SNACC_ARENA_LIMIT", str(arena_limit))
    a = CliRunner().invoke(cli_mod.cli, [str(d), "-o", "gpu.csv", "-c", "bzip2", "--no-show-progress", "--no-log"])
    assert a.exit_code == 0, (a.output, a.exception)
    assert made and made[0].calls, "-c bzip2 did not take the GPU route"
    assert ("pairs_list" in made[0].calls) == bool(arena_limit)
    assert made[0].options.get("defer_singles") == 1                 # a bzip2 run never needs the lz4 phase A
    monkeypatch.delenv("SNACC_ARENA_LIMIT", raising=False)
    monkeypatch.setenv("SNACC_BZIP2", "stdlib")
    n_made = len(made)
    b = CliRunner().invoke(cli_mod.cli, [str(d), "-o", "cpu.csv", "-c", "bzip2", "-n", "4", "--no-show-progress", "--no-log"])
    assert b.exit_code == 0, b.output
    assert len(made) == n_made, "SNACC_BZIP2=stdlib must take the thread-pool flow"
    assert (tmp_path / "gpu.csv").read_text() == (tmp_path / "cpu.csv").read_text()


def test_bzip2_save_compression_keeps_the_thread_pool_flow(tmp_path, monkeypatch, routed):
    cli_mod, made = routed
    d = _fasta_dir(tmp_path / "fa", k=3)
    blobs = tmp_path / "blobs"
    blobs.mkdir()
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SNACC_BZIP2", raising=False)
    r = CliRunner().invoke(cli_mod.cli, [str(d), "-o", "s.csv", "-c", "bzip2", "-s", str(blobs), "--no-show-progress", "--no-log"])
    assert r.exit_code == 0, r.output
    assert not made
    assert len(list(blobs.glob("*.bz2"))) == 3 + 9


def test_bzip2_is_a_gpu_algorithm_and_row_weights_follow_the_last_block():
    from snacc_amd.distributed import bzip2_row_weights, shard_rows_weighted
    from snacc_amd.pairwise_ncd import GPU_ALGORITHMS
    assert "bzip2" in GPU_ALGORITHMS
    w = bzip2_row_weights([899981 + 10, 899981 * 2, 500000, 10])
    assert w[1] < w[0] < w[2] and w[3] == w[0]                     # whole blocks of x come from the singles pass
    cuts = shard_rows_weighted(w, 2)
    assert cuts[0][0] == 0 and cuts[-1][1] == 4
