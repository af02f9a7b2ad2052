"""Test-side restatement of fhe-util's three transcoders (crates/fhe-util/src/lib.rs:71-190: transcode_to_bytes,
transcode_from_bytes, transcode_bidirectional) as the one operation they are: the low in_bits of each input element laid
end to end, least significant bit first; output element k is bits [k out_bits, (k + 1) out_bits) of that stream, bits
past its end read as zero; ceil(nin in_bits / out_bits) output elements.  A byte string is in_bits = 8.
tests/test_transcode_ref.py pins it against the oracle's transcode_from_bytes / transcode_to_bytes."""


def count(nin, in_bits, out_bits):
    return -(-(nin * in_bits) // out_bits)


def transcode(a, in_bits, out_bits):
    assert 0 < in_bits <= 64 and 0 < out_bits <= 64
    nout = count(len(a), in_bits, out_bits)
    # the stream as a string of binary digits, most significant (= last) bit first, zero-extended to nout whole elements
    # (slices of a string: linear in the length, where shifts of one big integer would be quadratic)
    bits = "".join(format(int(x) & ((1 << in_bits) - 1), "0%db" % in_bits) for x in reversed(a)).rjust(nout * out_bits, "0")
    return [int(bits[len(bits) - (k + 1) * out_bits:len(bits) - k * out_bits], 2) for k in range(nout)]
