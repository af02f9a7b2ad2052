"""The multiparty share kernels beyond the stock parameter sets, on the kernel sources under host emulation: the matrix
shapes of tests/devop_shapes.py up to N = 2048 through mbfv_shape_cases.case_shape (every word of every share against the
restatement, level 0 and the deepest level, the relin rounds on).  tests/test_mbfv_shapes_gpu.py runs the whole matrix
(and what only the hardware shows: which instance a launch took) on the MI355X, and with it the batches that span launch
groups: the smallest of them, 65537 items of N = 8, takes the emulation longer per share than this whole file."""
import pytest

import devop_cases as D
import devop_shapes as S
import mbfv_shape_cases as M
from helpers import load_engine

MAX_N = 2048
N_MATRIX = 2 * 9


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


_matrix = []


def matrix():
    if not _matrix:
        _matrix.extend(s for s in S.matrix_shapes() if s[0] <= MAX_N)
        assert len(_matrix) == N_MATRIX
    return _matrix


@pytest.mark.parametrize("i", range(N_MATRIX))
def test_matrix_shape(fhe, i):
    shp = matrix()[i]
    M.case_shape(fhe, False, shp)
    if D.mbfv_f64_eligible(shp):   # (none below N = 4096: kept for symmetry with tests/test_devop_shapes_emu.py)
        fhe.set_f64(False)
        try:
            M.case_shape(fhe, False, shp)
        finally:
            fhe.set_f64(True)
