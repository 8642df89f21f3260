"""CPU: the host half of the keyed refine-pass draw (`apply.PhiloxCloud`, `genie_refine_cloud`): the C ABI symbol is declared, bound and
exported; `PhiloxCloud.host` is the numpy generator statement; a pure-Python Philox4x64-10 written here with the constants and the
counter convention the kernel is written to equals numpy (large key words, a large counter word 1, block counts that cross a word
boundary); the sweep constant of the host mirrors the kernel's grid cap; `source_parallel` without `ftrns2_device` is still refused."""
import os
import re
import types

import numpy as np
import pytest

from genie_amd import _lib, apply, postproc

M64 = (1 << 64) - 1
MUL0, MUL1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
WEYL0, WEYL1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def philox4x64_10(ctr, key):
    """One block: ten rounds of [hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0] with hi0:lo0 = M0 * c0 and hi1:lo1 = M1 * c2, the key bumped
    by the Weyl constants after every round."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = MUL0 * c0, MUL1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & M64, (p0 >> 64) ^ c3 ^ k1, p0 & M64
        k0, k1 = (k0 + WEYL0) & M64, (k1 + WEYL1) & M64
    return c0, c1, c2, c3


def draw_python(key, source, n_elem):
    """Flat element j = word j % 4 of the block whose counter is (j // 4 + 1, source, 0, 0), as a double (u >> 11) * 2**-53."""
    out = np.empty(n_elem, dtype=np.float64)
    for b in range((n_elem + 3) // 4):
        words = philox4x64_10((b + 1, source, 0, 0), key)
        for k in range(min(4, n_elem - 4 * b)):
            out[4 * b + k] = (words[k] >> 11) * (1.0 / 9007199254740992.0)
    return out


def draw_numpy(key, source, shape):
    bits = np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array([0, source, 0, 0], dtype=np.uint64))
    return np.random.Generator(bits).random(shape)


def test_refine_cloud_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    assert re.search(r"\bint\s+genie_refine_cloud\s*\(", header), "genie_refine_cloud is not declared in genie_hip.h"
    assert "genie_refine_cloud" in {n for n, _, _ in _lib.SYMBOLS}, "genie_refine_cloud is not in _lib.SYMBOLS"
    fn = _lib.load().genie_refine_cloud
    assert fn.restype is not None and len(fn.argtypes) == 17


def test_host_sweep_constant_mirrors_the_kernels_grid_cap():
    src = open(os.path.join(_lib.REPO, "genie_amd", "csrc", "cloud_kernels.hpp")).read()
    block = int(re.search(r"constexpr int RC_BLOCK = (\d+);", src).group(1))
    cap = int(re.search(r"constexpr int RC_MAX_WG = (\d+);", src).group(1))
    assert postproc.REFINE_CLOUD_SWEEP == block * cap * 4


@pytest.mark.parametrize("key", [(0, 0), (M64, (1 << 63) + 5), (1 << 63, 12345), (0x0123456789ABCDEF, 0xFEDCBA9876543210)])
@pytest.mark.parametrize("source", [0, 1, (1 << 32) + 7, M64])
def test_pure_python_philox_equals_numpy(key, source):
    for n_elem in (1, 3, 4, 5, 8, 9, 15):                # within one block, exactly at a block's end, one word into the next
        got, want = draw_python(key, source, n_elem), draw_numpy(key, source, n_elem)
        assert got.tobytes() == want.tobytes(), (key, source, n_elem)
    assert draw_python(key, source, 15).tobytes() == draw_numpy(key, source, (5, 3)).tobytes()          # [n, 3] is the flat order


def test_numpy_counter_convention_of_the_issue():
    """`philox_next` increments counter word 0 before it generates: a generator started at counter 10 hands out blocks 11 and 12."""
    got = np.random.Generator(np.random.Philox(key=[5, 7], counter=[10, 0, 0, 0])).random(8)
    want = [(w >> 11) * 2.0 ** -53 for c in (11, 12) for w in philox4x64_10((c, 0, 0, 0), (5, 7))]
    assert got.tobytes() == np.array(want).tobytes()


@pytest.mark.parametrize("key,words", [((3, 4), (3, 4)), (5, (5, 0)), ((1 << 64) + 9, (9, 1)), ((1 << 128) - 1, (M64, M64)),
                                       (np.array([M64, 1 << 63], dtype=np.uint64), (M64, 1 << 63))])
def test_philox_cloud_host_is_the_numpy_statement(key, words):
    pc = apply.PhiloxCloud(key)
    assert pc.key == words
    np_key = key if isinstance(key, int) else np.asarray(key, dtype=np.uint64)
    for source, n in ((0, 1), (2, 7), ((1 << 32) + 7, 300)):
        want = np.random.Generator(np.random.Philox(key=np_key, counter=[0, source, 0, 0])).random((n, 3))
        got = pc.host(source, n)
        assert got.dtype == np.float64 and got.shape == (n, 3) and got.tobytes() == want.tobytes()
        assert pc.host(source, n).tobytes() == got.tobytes()                    # nothing is stateful
    assert pc.host(0, 5).tobytes() != pc.host(1, 5).tobytes()
    assert pc.host(3, 0).shape == (0, 3)


@pytest.mark.parametrize("bad", [-1, 1 << 128, (1, 2, 3), (1,), (-1, 0), (0, 1 << 64)])
def test_philox_cloud_refuses_a_bad_key(bad):
    with pytest.raises(ValueError):
        apply.PhiloxCloud(bad)


def test_philox_cloud_with_source_parallel_still_needs_ftrns2_device():
    legs = [types.SimpleNamespace(net=types.SimpleNamespace(is_sharded=False))]      # no device: the checks come first
    with pytest.raises(ValueError, match="ftrns2_device"):
        apply.refine_sources(legs, None, np.zeros((4, 5)), None, None, 1.0, None, None, 10, None, None, None, None, None,
                             rand=apply.PhiloxCloud((1, 2)), source_parallel=(0, 2))
