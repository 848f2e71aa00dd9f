"""The packed offset slab of the folded fp16 head (csrc/gruhead.hip, HIMO_HEAD_PACKED_SLAB), restated in numpy float16 -- CPU only.

The folded matrices keep the packer's ordinary layout [slab][term][cout][16] (term 0 = hi, term 1 = lo of the x64-scaled rows); the
kernel puts the ninth slab's B fragment together from it in registers -- the lanes of k 0-7 take rows 0-3 of the hi plane twice, the
lanes of k 8-15 rows 0-3 of the lo plane twice -- and writes the A columns hi(o, 1) | lo(o, 1) | hi(o, 1) | 0.  Checked here:
the rows so assembled are hi / lo of the x64-scaled folded rows computed independently, and the one K = 16 product equals the three
kept terms hi hi + lo hi + hi lo of the three-term slab, term by term.
"""
import numpy as np

import head_oracle as ho


def _split16(x):
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _packer_planes(F144):
    """the two 16-bit planes of himo_conv_pack_weights_ex(packed_format 1) for a [144][cout] matrix, as [slab][term][cout][16]"""
    hi, lo = _split16(F144.astype(np.float32) * np.float32(64.0))
    cout = F144.shape[1]
    return np.stack([hi.reshape(9, 16, cout).transpose(0, 2, 1), lo.reshape(9, 16, cout).transpose(0, 2, 1)], 1)


def _kernel_b_fragment(planes, col):
    """what gemm192's packed path loads for output column ``col``: for k-half lh the first 8 bytes of plane lh, repeated"""
    rec = planes[8]                                    # [term][cout][16]
    return np.concatenate([rec[0, col, :4], rec[0, col, :4], rec[1, col, :4], rec[1, col, :4]])


def _kernel_a_row(o):
    """the ninth slab's plane 0 for one point: thread q = 0..3 writes hi | lo | hi | zeros of (o0, o1, o2, 1)"""
    hi, lo = _split16(np.array([o[0], o[1], o[2], 1.0], np.float32))
    return np.concatenate([hi, lo, hi, np.zeros(4, np.float16)])


def test_packed_rows_are_hi_and_lo_of_the_scaled_folded_rows():
    W = ho.weights(0, 1.0)
    for k in ("wzr", "wq", "w1"):
        F = ho.fold(W["w_off"], W["b_off"], W[k]).float().numpy()
        planes = _packer_planes(F)
        rows = F[128:132].astype(np.float64) * 64.0                      # independently: the four folded rows, scaled
        hi = rows.astype(np.float16)
        lo = (rows - hi.astype(np.float64)).astype(np.float16)
        assert np.abs(lo.astype(np.float64)).max() > 0
        for col in (0, 1, 31, F.shape[1] - 1):
            b = _kernel_b_fragment(planes, col)
            assert np.array_equal(b[0:4], hi[:, col]) and np.array_equal(b[4:8], hi[:, col]) and np.array_equal(b[8:12], lo[:, col])
            assert not planes[8][:, col, 4:].any()                        # rows 4-15 of the slab are zero: k 12-15 may repeat anything
        assert np.array_equal(planes[8][0, :, :4].T.astype(np.float64) + planes[8][1, :, :4].T.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))


def test_one_packed_product_is_the_three_kept_terms():
    W = ho.weights(0, 1.0)
    F = ho.fold(W["w_off"], W["b_off"], W["wq"]).float().numpy()
    planes = _packer_planes(F)
    rng = np.random.default_rng(5)
    for o in (np.array([0.1, -0.1, 3.0]), np.zeros(3), rng.uniform(-0.1, 0.1, 3), np.array([0.0999755859375, 0.05, -2.999])):
        a = _kernel_a_row(o.astype(np.float32)).astype(np.float64)
        assert not a[12:].any()
        ahi, alo = (t.astype(np.float64) for t in _split16(np.array([*o, 1.0], np.float32)))
        for col in (0, 17, 127):
            b = _kernel_b_fragment(planes, col).astype(np.float64)
            bhi, blo = planes[8][0, col, :4].astype(np.float64), planes[8][1, col, :4].astype(np.float64)
            products = a * b                                           # fp16 x fp16 products are exact in float64
            assert np.array_equal(products[0:4], ahi * bhi) and np.array_equal(products[4:8], alo * bhi) and np.array_equal(products[8:12], ahi * blo)
            assert not products[12:].any()
