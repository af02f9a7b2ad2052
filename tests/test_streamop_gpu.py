"""The streaming kernels at their accumulator, rounding and shape edges on the MI355X (the HIP build): the cases of
tests/streamop_cases.py word for word against the Python-int restatements of tests/streamop_ref.py, each with the
profiler on, and the census of the module: dot_kernel<1> for one part and dot_kernel<2> for more, the word kernels of the
wire format for rows of 128 coefficients and more between 16-byte aligned buffers and the byte kernels otherwise, and all
ten symbols over the module."""
import re

import numpy as np
import pytest

import keyed_cases as K
import streamop_cases as S
from helpers import HIP_LIB, Xfer, load_engine

pytestmark = pytest.mark.gpu

CENSUS = ("dot_kernel<1>", "dot_kernel<2>", "mul_plain_kernel", "switch_down_kernel", "substitute_kernel", "wire_pack_kernel",
          "wire_unpack_kernel", "wire_pack_words_kernel", "wire_unpack_words_kernel", "ks_mac_kernel")


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


_seen = {}   # test key -> the census symbols its run launched


def launched(fhe, key, call):
    """The census symbols among the kernels call() launches (the engine's profiler), remembered under `key`."""
    symbols = K.kernels_of(fhe, call)
    got = {name for name in CENSUS if any(re.search(r"\b" + re.escape(name) + r"\(", s) for s in symbols)}
    _seen.setdefault(key, set()).update(got)
    return got


def only(got, family, want):
    """Of the census symbols that start with `family`, exactly `want` ran."""
    assert {s for s in got if s.startswith(family)} == set(want), (sorted(got), family, want)


# ---- dot product ---------------------------------------------------------------------------------------------------------
def run_dot_group(fhe, name, group):
    for i, case in enumerate(S.dot_cases(name, group)):
        got = launched(fhe, ("dot", name, group), lambda: S.run_dot(fhe, (True, "abi", False)[i % 3], case))
        only(got, "dot_kernel", ["dot_kernel<1>" if case.parts == 1 else "dot_kernel<2>"])


@pytest.mark.parametrize("group", S.DOT_GROUPS)
@pytest.mark.parametrize("name", list(S.DOT_CONTEXTS))
def test_dot(fhe, name, group):
    run_dot_group(fhe, name, group)


# ---- ct x pt, modulus switching, substitution ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.MUL_PLAIN_N)
def test_mul_plain(fhe, n):
    assert "mul_plain_kernel" in launched(fhe, ("mul_plain", n), lambda: S.case_mul_plain(fhe, True, n))


@pytest.mark.parametrize("name", list(S.SD_SETS))
def test_switch_down(fhe, name):
    assert "switch_down_kernel" in launched(fhe, ("switch_down", name), lambda: S.case_switch_down(fhe, True, name))


@pytest.mark.parametrize("n", S.SUB_N)
def test_substitute(fhe, n):
    assert "substitute_kernel" in launched(fhe, ("substitute", n), lambda: S.case_substitute(fhe, True, n))


def test_host_arrays_and_device_arrays(fhe):
    """The smallest of each through numpy arrays and through DeviceArrays."""
    for dev in (False, "abi"):
        S.case_mul_plain(fhe, dev, 8)
        S.case_switch_down(fhe, dev, "62-62-20")
        S.case_substitute(fhe, dev, 8)


# ---- wire format ---------------------------------------------------------------------------------------------------------
def run_wire(fhe, widths, n, dev=True):
    for off in S.WIRE_OFFSETS:
        got = launched(fhe, ("wire", widths, n, off), lambda: S.case_wire(fhe, dev, widths, n, offsets=(off,)))
        # (every run makes the wrappers' calls on the allocator's aligned buffers first: those follow the row length alone)
        aligned = ["wire_pack_words_kernel", "wire_unpack_words_kernel"] if n >= 128 else ["wire_pack_kernel", "wire_unpack_kernel"]
        here = (["wire_pack_words_kernel", "wire_unpack_words_kernel"] if S.wire_word_kernels(n, off)
                else ["wire_pack_kernel", "wire_unpack_kernel"])
        only(got, "wire_", set(aligned) | set(here))
    # the offset buffers alone: what launch_wire picks for them
    from fhe_rs_amd import api
    x = Xfer(dev)
    c = fhe.Context(list(S.wire_moduli(widths, n)), n)
    pb, _ntt, data = S.wire_data(widths, n)
    for off in S.WIRE_OFFSETS:
        base, view = S.byte_view(fhe, x, data, off)
        out, src = x.to(np.zeros_like(pb)), x.to(pb)

        def calls():
            assert K.raw(fhe, "fhe_poly_deserialize_dev", c._h, api._dptr8(view), api._dptr(out), len(pb), 0, api._stream())[0] == 0
            assert K.raw(fhe, "fhe_poly_serialize_dev", c._h, api._dptr(src), api._dptr8(view), len(pb), 0, api._stream())[0] == 0
            K.same(x.back(out), pb, ("deserialize", widths, n, off))
        got = launched(fhe, ("wire alone", widths, n, off), calls)
        only(got, "wire_", ["wire_pack_words_kernel", "wire_unpack_words_kernel"] if S.wire_word_kernels(n, off)
             else ["wire_pack_kernel", "wire_unpack_kernel"])


@pytest.mark.parametrize("n", S.WIRE_N)
@pytest.mark.parametrize("widths", S.WIRE_CONTEXTS, ids=lambda w: "-".join(map(str, w)))
def test_wire(fhe, widths, n):
    run_wire(fhe, widths, n)


@pytest.mark.parametrize("dev", [False, "abi"], ids=["host", "abi"])
def test_wire_other_forms(fhe, dev):
    for n in S.WIRE_N:
        S.case_wire(fhe, dev, S.WIRE_MIXED, n)


# ---- seventeen digits at the top -----------------------------------------------------------------------------------------
def test_seventeen_digits_at_the_top_keyed(fhe):
    symbols = K.kernels_of(fhe, lambda: S.case_top17_keyed(fhe, True))
    assert any("ks_mac_keyed_kernel" in s for s in symbols), symbols


@pytest.mark.parametrize("mode", ["UNFUSED", "FUSED"])
def test_seventeen_digits_at_the_top_plain(fhe, mode):
    got = launched(fhe, ("top17", mode), lambda: S.case_top17_plain(fhe, True, getattr(fhe.KeySwitchingKey, mode)))
    assert ("ks_mac_kernel" in got) == (mode == "UNFUSED"), sorted(got)


def test_seventeen_digits_at_the_top_hoisted(fhe):
    symbols = K.kernels_of(fhe, lambda: S.case_top17_hoisted(fhe, True))
    assert any("hoist_mac_kernel" in s for s in symbols), symbols


# ---- census --------------------------------------------------------------------------------------------------------------
def test_census(fhe):
    """The union over the module names all ten kernels (what did not run in this process yet -- a selected or distributed
    run -- runs here in its smallest form)."""
    seen = lambda: set().union(*_seen.values()) if _seen else set()   # noqa: E731
    if not {"dot_kernel<1>", "dot_kernel<2>"} <= seen():
        run_dot_group(fhe, "n8-62-61-60", "parts")
    if "mul_plain_kernel" not in seen():
        launched(fhe, ("mul_plain", 8), lambda: S.case_mul_plain(fhe, True, 8))
    if "switch_down_kernel" not in seen():
        launched(fhe, ("switch_down", "50-62"), lambda: S.case_switch_down(fhe, True, "50-62"))
    if "substitute_kernel" not in seen():
        launched(fhe, ("substitute", 8), lambda: S.case_substitute(fhe, True, 8))
    if not {s for s in CENSUS if s.startswith("wire_")} <= seen():
        run_wire(fhe, (33,), 128)
    if "ks_mac_kernel" not in seen():
        launched(fhe, ("top17", "UNFUSED"), lambda: S.case_top17_plain(fhe, True, fhe.KeySwitchingKey.UNFUSED))
    assert sorted(set(CENSUS) - seen()) == []
