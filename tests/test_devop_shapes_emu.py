"""Device encode, encrypt and key generation beyond the stock parameter sets, on the kernel sources under host
emulation: the matrix shapes of tests/devop_shapes.py up to N = 2048, the round-trip pins (two of them at N = 4096),
and the first 16 shapes of the `devops` sweep family (N up to 16384).  tests/test_devop_shapes_gpu.py runs the whole
matrix (and what only the hardware shows: which instance a launch took) on the MI355X."""
import pytest

import devop_cases as D
import devop_shapes as S
import encrypt_cases as X
from helpers import load_engine

MAX_N = 2048   # (the five matrix shapes at N = 4096 take longer here than the three families' own emulated files together)
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
    first_of_logm = i == min(j for j, s in enumerate(matrix()) if s[0] == shp[0])
    D.check_shape(fhe, False, shp, host_handle=first_of_logm)
    if D.f64_eligible(shp):
        fhe.set_f64(False)
        try:
            D.check_shape(fhe, False, shp)
        finally:
            fhe.set_f64(True)


@pytest.mark.parametrize("i", range(3), ids=["general", "class3", "t61"])
def test_roundtrip(fhe, i):
    opar, par = D.params(fhe, S.roundtrip_shapes()[i])
    X.case_roundtrip(fhe, False, opar, par, level=0)


@pytest.mark.parametrize("idx", range(16))
def test_random_shape(fhe, idx):
    D.check_random_shape(fhe, False, idx)
