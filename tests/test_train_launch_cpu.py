"""CPU: the context-free size functions of the training backward's scratch. Every per-wave partial slot is `n_acc` accumulator tiles
of 256 floats, `n_vec` bias vectors of 16 and 16 scalars; the sizes below were measured on the build before the host launchers
of the training backward were merged and pin that layout (a caller allocates by them, the kernels index by them)."""
import os

import pytest

from genie_amd import _lib


@pytest.fixture(scope="module")
def lib():
    src_dir = os.path.dirname(_lib.SRC)
    newest = max(os.path.getmtime(os.path.join(src_dir, f)) for f in os.listdir(src_dir))
    if not os.path.exists(_lib.LIB_PATH) or os.path.getmtime(_lib.LIB_PATH) < newest:
        _lib.build()
    return _lib.load()


def test_gradient_blob_floats(lib):
    assert lib.genie_train_grad_floats() == 65816


@pytest.mark.parametrize("n_picks,floats", [(1, 8448), (17, 8448), (64, 8448), (65, 16896), (10240, 1351680), (10241, 1351680),
                                            (100000, 1351680)])
def test_lslc_backward_partial_floats(lib, n_picks, floats):
    """One workgroup of four waves per 64 picks, at most 160 workgroups; (8 * 256 + 3 * 16 + 16) floats per wave."""
    assert lib.genie_lslc_bwd_part_floats(n_picks) == floats


@pytest.mark.parametrize("shape,floats", [((1, 1, 1), 12946048), ((3, 17, 5), 12956800), ((7, 400, 33), 13183936),
                                          ((40, 2000, 200), 19696640)])
def test_arrivals_backward_scratch_floats(lib, shape, floats):
    assert lib.genie_arrivals_bwd_scratch_floats(*shape) == floats


def test_arrivals_backward_scratch_of_an_empty_problem_is_zero(lib):
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.genie_arrivals_bwd_scratch_floats(*shape) == 0


def test_arrivals_training_save_floats(lib):
    assert lib.genie_arrivals_train_save_floats(3, 17) == 3264
