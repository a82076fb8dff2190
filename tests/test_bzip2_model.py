"""The CPU model of bzip2 (tests/bz2_model.py) against the codec the reference calls: real bytes equal to
bz2.compress (the first differing bit names the faulty stage), sizes from block bits, the pair composition the
kernels use, and the kernels' own per-block stages (snacc_amd/csrc/snk_bzip2.hip.h) compiled by g++."""
import bz2
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bz2_model as m

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = Path(__file__).resolve().parents[1]


def _acgt(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def _rle_len(data):
    return sum(len(u[2]) for u in m.rle1_units(data))


def _check_bytes(data, exact=True):
    got, want = m.compress(data), bz2.compress(data)
    assert len(got) == len(want) == m.size(data)
    if exact:
        assert got == want
    assert bz2.decompress(got) == data


SMALL = [b"", b"a", b"ab", bytes(range(256)), bytes(range(256))[::-1] * 3]
SMALL += [b"x" * k for k in (1, 2, 3, 4, 5, 254, 255, 256, 257, 258, 259, 260, 510, 511, 512, 1000)]
SMALL += [b"ACGT" + b"G" * k + b"TTA" for k in (3, 4, 255, 256, 259)]
SMALL += [bytes(np.random.default_rng(1).integers(0, 256, 5000, dtype=np.uint8)),
          _acgt(2, 20000), _acgt(3, 20000).lower(), b"ACGTRYKMSWBDHVN" * 300 + _acgt(4, 3000),
          bytes(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[np.random.default_rng(5).integers(0, 20, 30000)])]


def _periodic(block):
    """A block with tied rotations is a power of a shorter string."""
    n = len(block)
    return any(n % d == 0 and block == block[:d] * (n // d) for d in range(1, n))


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_small_inputs_byte_exact(k):
    _check_bytes(SMALL[k], exact=not any(_periodic(m.block_bytes(b)) for b in m.blocks(SMALL[k])))


@pytest.mark.parametrize("data", [b"ACGT" * 5000, b"AC" * 7001, b"N" * 100000, (b"ACGTN" * 7 + b"A" * 300) * 200], ids=["acgt", "ac", "n", "mixed"])
def test_whole_block_periodic_inputs_same_size(data):
    _check_bytes(data, exact=False)           # tied rotations move origPtr only


def _nmtf_input(target):
    """An input whose single block has exactly `target` MTF symbols (distinct bytes cycle, no runs)."""
    lo, hi = 1, target
    pool = bytes(np.random.default_rng(target).integers(0, 256, 2 * target + 100, dtype=np.uint8))
    gen = lambda n: pool[:n]                                                    # noqa: E731
    count = lambda d: m.mtf(m.bwt(d)[0], sorted(set(d))).size                    # noqa: E731
    while lo < hi:
        n = (lo + hi) // 2
        if count(gen(n)) < target:
            lo = n + 1
        else:
            hi = n
    for n in sorted(range(max(1, lo - 40), lo + 40), key=lambda k: abs(k - lo)):
        if count(gen(n)) == target:
            return gen(n)
    raise AssertionError(f"no input with nMTF {target}")


@pytest.mark.parametrize("target", [199, 200, 599, 600, 1199, 1200, 2399, 2400])
def test_group_count_thresholds(target):
    d = _nmtf_input(target)
    n_mtf = m.mtf(m.bwt(d)[0], sorted(set(d))).size
    assert n_mtf == target
    _check_bytes(d)


def _rescale_input():
    """Geometric byte frequencies (ratio 1/2 over 20 letters) plus 300 rare bytes: the winning table's counts build a
    Huffman tree deeper than 17, so BZ2_hbMakeCodeLengths rescales them."""
    rng = np.random.default_rng(3)
    p = 0.5 ** np.arange(20)
    d = rng.choice(20, 600000, p=p / p.sum()).astype(np.uint8) + 65
    d[rng.integers(0, d.size, 300)] = rng.integers(128, 256, 300)
    return d.tobytes()


def test_frequency_skew_forces_the_length_limit_rescale(monkeypatch):
    data = _rescale_input()
    assert len(m.blocks(data)) == 1
    fired = []
    build = m.make_code_lengths

    def counting(freq, max_len=m.MAX_LEN):
        fired.append(max(build(freq, 99)) > max_len)          # the same tree without the limit: deeper than 17?
        return build(freq, max_len)

    monkeypatch.setattr(m, "make_code_lengths", counting)
    _check_bytes(data)
    assert any(fired), "the input no longer reaches the maxLen-17 rescale"


def _runless(seed, n):
    """ACGT without two equal neighbours: its RLE1 stream is itself."""
    step = np.random.default_rng(seed).integers(1, 4, n)
    return ACGT[np.cumsum(step) % 4].tobytes()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_rle1_length_at_the_block_cut(delta):
    data = _runless(8, m.NBLOCK_MAX + delta)
    assert _rle_len(data) == m.NBLOCK_MAX + delta
    assert len(m.blocks(data)) == (2 if delta > 0 else 1)      # a full block at the end is not followed by an empty one
    _check_bytes(data)


def test_three_blocks_and_a_run_across_the_cut():
    x = _acgt(9, 899970) + b"G" * 300 + _acgt(10, 900000) + b"T" * 600
    assert len(m.blocks(x)) == 3
    assert m.size(x) == len(bz2.compress(x))


def _pair_set():
    big = _acgt(20, 899975) + b"A" * 255
    return [big, _acgt(21, 4000) + b"C" * 3, b"C" + _acgt(22, 3000), b"A" * 300 + _acgt(23, 2000) + b"AAA", b"", b"A"]


def test_pair_composition_equals_the_codec():
    seqs = _pair_set()
    kept = {}
    for i, x in enumerate(seqs):
        bx = m.blocks(x)
        kept[i] = [m.block_bits(m.block_bytes(b)) for b in bx[:-1]]
        assert m.stream_size(kept[i] + ([m.block_bits(m.block_bytes(bx[-1]))] if bx else [])) == len(bz2.compress(x))
    for i, x in enumerate(seqs):
        for j, y in enumerate(seqs):
            if len(x) + len(y) > 2000000:
                continue
            assert m.pair_size(x, y, kept[i]) == len(bz2.compress(x + y)), (i, j)


def test_x_ending_exactly_at_a_block_cut():
    x = _acgt(24, 899990)
    while m.blocks(x) and sum(len(u[2]) for u in m.blocks(x)[0]) < m.NBLOCK_MAX:
        x += b"A"
    x = x[: m.blocks(x)[0][-1][1]]             # x's raw input ends with the unit that fills its first block
    y = _acgt(25, 3000)
    assert m.pair_size(x, y) == len(bz2.compress(x + y))


# ---- the kernels' per-block stages, compiled for the host ---------------------------------------------------------
@pytest.fixture(scope="module")
def stage_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("bzemu")
    src = d / "bz_emu.cpp"
    src.write_text('#include "snk_bzip2.hip.h"\n#include <vector>\n'
                   'extern "C" unsigned long long bz_bits(const unsigned char *last, int n, int chunks) {\n'
                   '  std::vector<uint16_t> mtfv(n + 1); std::vector<uint8_t> sel(BZ_MAX_SEL), pos(n + 1); static BzTables tb;\n'
                   '  return bz_block_bits_serial(last, n, mtfv.data(), sel.data(), tb, chunks, pos.data()); }\n')
    so = d / "bz_emu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", str(ROOT / "snacc_amd" / "csrc"),
                           "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.bz_bits.restype = ctypes.c_ulonglong
    lib.bz_bits.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    return lib


@pytest.mark.parametrize("data", [b"a", b"ab", bytes(range(256)), _acgt(30, 30000), _nmtf_input(200), _nmtf_input(2400),
                                  b"N" * 5000 + _acgt(31, 3000), b"ACGT" * 2000, bytes(np.random.default_rng(3).integers(0, 256, 40000, dtype=np.uint8))],
                         ids=["a", "ab", "all256", "acgt", "nmtf200", "nmtf2400", "nrun", "periodic", "random"])
def test_kernel_stage_functions_agree_with_the_model(stage_lib, data):
    for blk in m.blocks(data):
        block = m.block_bytes(blk)
        last, _ = m.bwt(block)
        want = m.block_bits(block)
        assert stage_lib.bz_bits(last, len(last), 0) == want
        for chunks in (1, 7, 256, 1000):                      # the kernel's MTF in chunks (256 = one per lane)
            assert stage_lib.bz_bits(last, len(last), chunks) == want, chunks


def test_kernel_stage_functions_through_the_length_limit_rescale(stage_lib):
    block = m.block_bytes(m.blocks(_rescale_input())[0])
    last, _ = m.bwt(block)
    want = m.block_bits(block)
    assert stage_lib.bz_bits(last, len(last), 0) == want
    assert stage_lib.bz_bits(last, len(last), 256) == want


def test_kernel_stage_functions_on_a_full_block(stage_lib):
    block = m.block_bytes(m.blocks(_acgt(32, 950000))[0])
    assert len(block) >= m.NBLOCK_MAX
    last, _ = m.bwt(block)
    want = m.block_bits(block)
    assert stage_lib.bz_bits(last, len(last), 0) == want
    assert stage_lib.bz_bits(last, len(last), 256) == want
