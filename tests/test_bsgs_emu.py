"""Baby-step/giant-step hoisted matrix-vector product (fhe_bfv_matvec_bsgs_dev, KeySet.matvec_bsgs, EvaluationKey.bsgs): the
kernel sources under host emulation against the restatement tests/bsgs_ref.py and the engine's own composition (hoisted
matrix-vector products, one-key hoisted rotations, additions), every shape up to N = 1024.  tests/test_bsgs_gpu.py runs the
same cases on the MI355X, counts the launches and adds the larger row kinds."""
import pytest

import bsgs_cases as M
from fhe_oracle import bfv as obfv
from helpers import load_engine

FORMS = [False, "abi"]   # numpy arrays (staged by the wrappers) and DeviceArrays
IDS = ["host", "abi"]


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_anchor(fhe, dev):
    """N = 16 over [62, 60, 55], baby exponents (1, 9), giant exponents (3, 3), batch 2: shared and per-item grids."""
    M.case_anchor(fhe, dev)


def test_reference_forms_hoistmv_refs_inner_sums(fhe):
    """bsgs_ref shares the baby rotations between the groups: its inner sums are hoistmv_ref.matvec's, group by group."""
    import numpy as np

    import bsgs_ref
    import hoistmv_ref
    from fhe_oracle.rq import NTT, Poly

    n, sizes = M.SMALL
    sy = M.K.Synthetic(fhe, obfv.generate_moduli(sizes, n), n, 2, 341)
    keys = [sy.oracle_key(r) for r in range(2)]
    g = np.random.default_rng(341)
    c0, c1 = (Poly(sy.octx, NTT, M.K.uniform(g, sy.q, n).tolist()) for _ in range(2))
    pts = M.K.uniform(g, sy.q, n, (3, 3)).tolist()
    got = bsgs_ref.inner_sums(c0, c1, keys, [3, 9], pts)
    assert len(got) == 3
    for row, (i0, i1) in zip(pts, got):
        assert (i0, i1) == hoistmv_ref.matvec(c0, c1, keys, [3, 9], row[1:], row[0])


def test_deepest_level(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    M.case_anchor(fhe, "abi", cl=1, kl=1, seed=302, variants=(False,))


def test_differs_from_the_flat_product_in_a_word(fhe):
    """The flat call over the composed exponents differs word for word."""
    M.case_anchor(fhe, "abi", seed=304, variants=(True,), flat=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_forms(fhe, dev):
    M.case_forms(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matrix_times_encrypted_vector(fhe, dev):
    M.case_matrix_vector(fhe, dev)


@pytest.mark.parametrize("ngiant", [2, 4], ids=["G3", "G5"])
def test_every_tile_instance_and_its_tail(fhe, ngiant):
    M.case_tiles(fhe, "abi", ngiant)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_giant_groups(fhe, dev):
    M.case_giant_groups(fhe, dev)


def test_baby_fold_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, nbaby = 17, ngiant = 1, tile 2, every word at q_j - 1: the baby fold sees a
    seventeenth rotation after a fold, in both accumulator sets."""
    q = obfv.generate_moduli([62] * 16, 128)
    M.case_synthetic(fhe, "abi", q, 128, 17, 1, 1, seed=321, top=True, tile=2)


def test_giant_fold_at_the_top(fhe):
    """The same moduli, nbaby = 1, ngiant = 17 in one group: the carried giant accumulators pass sixteen products and
    sixteen addends."""
    q = obfv.generate_moduli([62] * 16, 128)
    M.case_synthetic(fhe, "abi", q, 128, 1, 17, 1, seed=323, top=True, rot_split=1)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128, nbaby = ngiant = 1: both digit loops fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    M.case_synthetic(fhe, "abi", q, 128, 1, 1, 1, seed=325, rot_split=1)


def test_grid_tail(fhe):
    """N = 1024 over three moduli, batch 1, nbaby = ngiant = 1: two lane chunks per row, six key ranges in a grid rounded
    up to eight."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    M.case_synthetic(fhe, "abi", q, 1024, 1, 1, 1, seed=327)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget(fhe, dev):
    M.case_w_budget(fhe, dev)


def test_table_limits(fhe):
    M.case_table_limits(fhe, "abi")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    M.case_refusals(fhe, dev)
