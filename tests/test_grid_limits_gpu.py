"""Batches past what one launch's grid holds in its second dimension (engine.hpp: GRID_YZ_MAX, launch_rows), on the
MI355X (the HIP build), at N = 16 over [62, 60, 55]: the calls that cut such a batch into launch groups (decrypt's phase,
expand_step) against the engine's own words for the same items in two smaller calls, with oracle ciphertexts planted in
the first and in the second group; and the calls that refuse such a batch, at the last batch they take and at the first
they refuse.  Inputs are uniform words below q_i, drawn on the device; every comparison is word for word.

Not reachable by a call: the limit of a grid's first dimension (2^31 blocks of 256 lanes do not fit the card)."""
import numpy as np
import pytest

import keyed_cases as K
from fhe_oracle import bfv as obfv
from helpers import HIP_LIB, arr, ct_arr, load_engine

pytestmark = pytest.mark.gpu

SMALL = (16, [62, 60, 55])
YZ = 65535          # engine.hpp GRID_YZ_MAX


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


@pytest.fixture(scope="module")
def setup(fhe):
    """The parameter set, one oracle client, and the shared inputs (never written): YZ + 2 uniform ciphertexts and
    YZ + 1 uniform plaintext polynomials."""
    import torch
    opar, par = K.params(fhe, *SMALL)
    cs = K.Clients(fhe, opar, par, 1, 211)
    gen = torch.Generator(device="cuda").manual_seed(2111)

    def uniform(*lead):
        rows = [torch.randint(0, int(q), lead + (opar.degree(),), dtype=torch.int64, device="cuda", generator=gen)
                for q in opar.moduli]
        return torch.stack(rows, dim=-2).contiguous()

    return opar, par, cs, uniform(YZ + 2, 2), uniform(YZ + 1)


def planted(cs, cts, at):
    """`cts` with fresh oracle ciphertexts at the indices `at`: (the new device array, {index: oracle ciphertext})."""
    import torch
    out, oracle = cts.clone(), {}
    for i in at:
        oracle[i] = cs.encrypt(0)
        out[i] = torch.from_numpy(ct_arr(oracle[i]).view(np.int64)).cuda()
    return out, oracle


def same(got, want, what):
    import torch
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), (what, "first differing word", int(torch.nonzero(got.reshape(-1) != want.reshape(-1))[0]))


def test_decrypt_past_one_group(fhe, setup):
    """65,537 ciphertexts: the phase takes two launch groups, the second of them two ciphertexts."""
    import torch
    opar, par, cs, cts, _ = setup
    batch = YZ + 2
    inp, oracle = planted(cs, cts[:batch], (0, YZ))
    s_ntt = torch.from_numpy(arr(cs.sk[0]._s(opar.ctx[0])).view(np.int64)).cuda()
    got = par.decrypt(s_ntt, inp)
    assert got.shape == (batch, opar.degree())
    same(got, torch.cat([par.decrypt(s_ntt, inp[:40000]), par.decrypt(s_ntt, inp[40000:])]), "decrypt in two calls")
    for i, c in oracle.items():
        assert got[i].cpu().numpy().view(np.uint64).tolist() == cs.sk[0].decrypt(c), ("oracle ciphertext", i)


def test_expand_past_one_group(fhe, setup):
    """32,769 ciphertexts to size 2: expand_step runs over 65,538 polynomials, three of them in its second group."""
    import torch
    opar, par, cs, cts, _ = setup
    n, batch = opar.degree(), (YZ + 3) // 2
    exps = fhe.EvaluationKey.exponents(n, expansion_level=1)
    ogk, gks = cs.galois_keys(exps)
    ek = fhe.EvaluationKey(n, gks[0])
    inp, oracle = planted(cs, cts[:batch], (0, batch - 1))
    got = ek.expands(inp, 2)
    assert got.shape == (2, batch) + tuple(inp.shape[1:])
    cut = batch // 2 + 1
    same(got, torch.cat([ek.expands(inp[:cut], 2), ek.expands(inp[cut:], 2)], dim=1), "expands in two calls")
    for i, c in oracle.items():
        want = obfv.expands(c, 2, ogk[0])
        for slot in range(2):
            assert np.array_equal(got[slot][i].cpu().numpy().view(np.uint64), ct_arr(want[slot])), ("oracle ciphertext", i, slot)


def refused(fhe, call):
    with pytest.raises(fhe.FheError) as err:
        call()
    assert err.value.code == -1 and "grid limit" in str(err.value), err.value


def test_add_plain_last_batch_and_refusal(fhe, setup):
    import torch
    opar, par, cs, cts, pts = setup
    ctx = par.context_at_level(0)
    refused(fhe, lambda: ctx.add_plain(cts[:YZ + 1], pts[:YZ + 1]))
    got, h = ctx.add_plain(cts[:YZ], pts[:YZ]), YZ // 2
    same(got, torch.cat([ctx.add_plain(cts[:h], pts[:h]), ctx.add_plain(cts[h:YZ], pts[h:YZ])]), "add_plain in two calls")
    assert not torch.equal(got[YZ - 1, 0], cts[YZ - 1, 0]) and torch.equal(got[YZ - 1, 1], cts[YZ - 1, 1])


def test_mul_plain_last_batch_and_refusal(fhe, setup):
    import torch
    opar, par, cs, cts, pts = setup
    ctx = par.context_at_level(0)
    refused(fhe, lambda: ctx.mul_plain(cts[:YZ + 1], pts[:YZ + 1]))
    got, h = ctx.mul_plain(cts[:YZ], pts[:YZ]), YZ // 2
    same(got, torch.cat([ctx.mul_plain(cts[:h], pts[:h]), ctx.mul_plain(cts[h:YZ], pts[h:YZ])]), "mul_plain in two calls")
    assert not torch.equal(got[YZ - 1], cts[YZ - 1])


def test_dot_product_last_batch_and_refusal(fhe, setup):
    """One two-part ciphertext and one plaintext per item (count = 1: the arrays are the shared ones, reshaped)."""
    import torch
    opar, par, cs, cts, pts = setup
    ctx = par.context_at_level(0)
    c, p = cts[:YZ + 1, None], pts[:YZ + 1, None]
    refused(fhe, lambda: ctx.dot_product_scalar(c, p))
    got, h = ctx.dot_product_scalar(c[:YZ], p[:YZ]), YZ // 2
    assert got.shape == cts[:YZ].shape
    same(got, torch.cat([ctx.dot_product_scalar(c[:h], p[:h]), ctx.dot_product_scalar(c[h:YZ], p[h:YZ])]),
         "dot_product_scalar in two calls")
    same(got, ctx.mul_plain(cts[:YZ], pts[:YZ]), "a dot product of one term is the product")
