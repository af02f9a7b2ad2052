"""tests/scaler_edge_cases.py on the MI355X (the HIP build): the scaler on columns that sit on its rounding thresholds
and walk its tables, bit for bit against the oracle, with the launched scale_kernel<NF, PLAIN, WIDE_W> instances read from
the profiler's kernel symbols:

* all 18 NF of ScaleNFs x {PLAIN, non-PLAIN} on their exact fit;
* WIDE_W at NF = 6, 27 and 64: 3/7 over 6 (the smallest count of 62-bit moduli at which scaler_upload's bound reaches
  2^191; 5 stay on the fast instance), 24 and 40 moduli of 62 bits, and 2/3 over 24, where t really passes 2^191;
* the instance each scaler was meant for (scaler_edge_inputs.instance_of, the host's bounds restated) is the one launched;
* one ciphertext of the stock n = 4096 set whose phase sits on the decryption scaler's thresholds, F64 on and off."""
import re

import pytest

import scaler_edge_cases as E
import scaler_edge_inputs as I
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu

# the cell table: (NF, kind) of every scale_kernel instance this file must launch
CELLS = [(nf, kind) for nf in I.SCALE_NFS for kind in ("plain", "full")] + [(6, "wide"), (27, "wide"), (64, "wide")]
_SYMBOL = re.compile(r"scale_kernel<(\d+), (true|false)(?:, (true|false))?>")
_launched = {}    # scaler name -> cells its run launched


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


def cell_of_symbol(symbol):
    m = _SYMBOL.search(symbol)
    if not m:
        return None
    return int(m.group(1)), "plain" if m.group(2) == "true" else "wide" if m.group(3) == "true" else "full"


def run_scaler(fhe, name, dev=True):
    sc = next(s for s in I.all_scalers() if s.name == name)
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        E.case_scaler(fhe, dev, sc)
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    cells = {cell_of_symbol(s) for s in symbols} - {None}
    assert cells == {I.instance_of(sc)}, (name, sorted(cells), I.instance_of(sc))
    _launched[name] = cells


@pytest.mark.parametrize("name", [s.name for s in I.all_scalers()])
def test_scaler_on_its_thresholds(fhe, name):
    run_scaler(fhe, name)


@pytest.mark.parametrize("name", ["one_3x59", "w37_6x62", "bfv4096_down"])
def test_scaler_on_its_thresholds_host_pointers(fhe, name):
    run_scaler(fhe, name, dev=False)


def test_every_instance_was_launched(fhe):
    """All 18 x {PLAIN, non-PLAIN} instances and WIDE_W at NF = 6, 27, 64 appear among the kernel symbols (scalers that did
    not run in this process yet -- a selected or distributed run -- run here)."""
    assert [c for c in CELLS if c[1] == "wide"] == sorted({I.instance_of(s) for s in I.all_scalers() if I.wide_w(s)})
    for sc in I.all_scalers():
        if sc.name not in _launched:
            run_scaler(fhe, sc.name)
    seen = set().union(*_launched.values())
    missing = sorted(set(CELLS) - seen)
    assert not missing, missing
    assert len(seen & set(CELLS)) == 2 * 18 + 3


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "integer"])
def test_decrypt_on_the_threshold(fhe, f64):
    fhe.set_f64(f64)
    try:
        E.case_decrypt_on_threshold(fhe, True)
    finally:
        fhe.set_f64(True)
