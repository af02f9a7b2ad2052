"""One shape of tests/devop_shapes.py through the encode, encrypt and key-generation cases (encode_cases,
encrypt_cases, keygen_cases), every item against the restatements bit for bit.  Shared by
tests/test_devop_shapes_gpu.py (the HIP build), tests/test_devop_shapes_emu.py (kernel sources under host emulation)
and the `devops` family of tests/random_sweep_gpu.py; the launch-group rule and the symbol parsers also serve
tests/test_mbfv_shapes_gpu.py.  `dev`: as helpers.Xfer."""
import re

import devop_shapes as S
import encode_cases as E
import encrypt_cases as X
import keygen_cases as G


def params(fhe, shp):
    n, sizes, t, variance, _batch = shp
    return G.params(fhe, n, t, moduli_sizes=sizes, variance=variance)


def check_encode(fhe, dev, shp, batches=(1, 3)):
    n = shp[0]
    opar, par = params(fhe, shp)
    levels = sorted({0, opar.max_level()})
    E.case_parity(fhe, dev, opar, par, batches=batches, nvalues_list=(0, 1, n // 2 + 3, n), levels=levels)
    E.case_parity(fhe, dev, opar, par, batches=batches[-1:], nvalues_list=(n // 2 + 3, n), levels=levels, seed=2, wide=True)


def check_encrypt(fhe, dev, shp):
    opar, par = params(fhe, shp)
    X.case_sampler_parity(fhe, dev, opar, par, (opar.variance,), batch=2)
    X.case_encrypt_parity(fhe, dev, opar, par, batch=shp[4])


def check_keygen(fhe, dev, shp, host_handle=False):
    opar, par = params(fhe, shp)
    if opar.max_level() == 0:   # one modulus: decomposition keys only; relinearization is KeySwitchingNotSupported
        key = G.case_galois(fhe, dev, opar, par, [3], 0, 0)[0]
        if host_handle:
            G.case_same_as_host_handle(fhe, dev, opar, par, key.ksk, exponent=key.exponent)
    else:
        rk = G.case_relin(fhe, dev, opar, par, 0, 0)
        if host_handle:
            G.case_same_as_host_handle(fhe, dev, opar, par, rk.ksk, relin=True)
    G.case_generic(fhe, dev, opar, par, 0, 0, nkeys=1)


def check_shape(fhe, dev, shp, host_handle=False, encode_batches=(1, 3)):
    check_encode(fhe, dev, shp, encode_batches)
    check_encrypt(fhe, dev, shp)
    check_keygen(fhe, dev, shp, host_handle)


def check_random_shape(fhe, dev, idx):
    """Shape idx of the `devops` sweep family (tests/random_sweep_gpu.py; its first indices are fixed tests)."""
    check_shape(fhe, dev, S.random_shape(idx), host_handle=idx % 8 == 0)


def launch_group(nmoduli, n, rows_per_item, batch, budget, cap=65535):
    """Items per launch group, engine.hpp's encrypt_group restated: the u64 scratch rows of one group (`rows_per_item`
    polynomials of nmoduli x n words per item) stay within `budget` bytes and `cap` items, and the batch is split
    into groups of equal size.  Secret-key encryption: 1 row per item in 1 GiB for whole rows (N <= 16384), 2 in
    256 MiB above; public-key encryption: one group of up to 65535 for whole rows, 3 rows in 256 MiB above; key
    generation: ndigits rows per key in 1 GiB for whole rows, 2 ndigits in 256 MiB above, at most 32 keys (KG_KEYS);
    the multiparty shares (mbfv_shares): 1 row per item and no byte budget for whole rows, so the cap of 65535 items
    alone splits a batch, and `edraws` rows per item (the transformed draws) in 256 MiB above."""
    per = max(1, rows_per_item) * nmoduli * n * 8
    most = max(1, min(cap, budget // per))
    groups = -(-batch // most)
    return -(-batch // groups)


def boundary_items(batch, group):
    """The first and last item of a batch and both neighbours of every boundary between launch groups of `group`."""
    cuts = range(group, batch, group)
    return sorted({0, batch - 1} | {c - 1 for c in cuts} | set(cuts))


KG_KEYS = 32


def f64_eligible(shp):
    """One of the shape's launches takes an F64 instance while the switch is on."""
    return any(kind.startswith("f64") for _k, _lm, kind in S.cells(shp))


_SYMBOL = re.compile(r"(\w+_kernel)<(\d+), (true|false), (\d+)>")


def cell_of_symbol(symbol):
    """A profiler entry's demangled kernel symbol, `...name_kernel<LOGM, NARROW, F64>(...)`, as a cell of
    devop_shapes.all_cells(); None for every other kernel."""
    m = _SYMBOL.search(symbol)
    if not m or m.group(1) not in S.KERNELS:
        return None
    hr = int(m.group(4))
    kind = "f64_%d" % hr if hr else "narrow" if m.group(3) == "true" else "general"
    return m.group(1), int(m.group(2)), kind


_MBFV_SYMBOL = re.compile(r"(mbfv_share_kernel)<(\d+), (true|false), (\d+), (\d+)>")


def mbfv_cell_of_symbol(symbol):
    """As cell_of_symbol for `...mbfv_share_kernel<LOGM, NARROW, F64, FORM>(...)`: a cell of
    devop_shapes.mbfv_all_cells(); None for every other kernel."""
    m = _MBFV_SYMBOL.search(symbol)
    if not m:
        return None
    hr = int(m.group(4))
    kind = "f64_%d" % hr if hr else "narrow" if m.group(3) == "true" else "general"
    return m.group(1), int(m.group(2)), kind, int(m.group(5))


def mbfv_f64_eligible(shp):
    """One of the shape's share launches takes an F64 instance while the switch is on."""
    return any(kind.startswith("f64") for _k, _lm, kind, _f in S.mbfv_cells(shp))


def chunk_group(batch, cap=65535):
    """Items per launch of the loops that cut a batch into chunks of `cap` with a tail (for_groups with a fixed size):
    public-key encryption of whole rows -- and with it the public-key-switch share -- and the aggregator mbfv_sum,
    whose polynomial index is the grid's second dimension."""
    return min(batch, cap)
