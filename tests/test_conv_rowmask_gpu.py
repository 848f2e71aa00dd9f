"""The row-masked 3x3 convolution (csrc/convsg.hip conv3_rowmask_kernel, HIMO_ACT_ROW_MASK) against the dense split-input kernel
on the same inputs: a pixel whose mask bit is set gets the dense kernel's value bit for bit, every other byte of the output keeps
the sentinel it was prefilled with, the input is not touched; descriptors the plan does not admit are refused with the documented
status and write nothing."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                                  # a quiet-NaN bit pattern no epilogue produces
EPI_BIAS, EPI_BIAS_BN_GELU = 0, 1


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import model  # noqa: F401  (registers the convolution entry points)
    return _lib.load()


def _stream():
    from himo_amd import _lib
    return _lib.stream_handle()


def split_encode(x):
    """float32 [..., C] (C % 16 == 0) -> int32 words of the split activation format"""
    h = x.half()
    l = (x - h.float()).half()
    g = x.shape[-1] // 16
    rec = torch.stack([h.reshape(*x.shape[:-1], g, 16), l.reshape(*x.shape[:-1], g, 16)], -2).reshape(*x.shape[:-1], 2 * x.shape[-1])
    return rec.view(torch.int32)


def pack_mask(m: np.ndarray, words: int) -> torch.Tensor:
    """bool [n][rows][w] -> int64 [n][words]: bit c of word k = pixel 64 k + c, pixels numbered row * w + column"""
    n = m.shape[0]
    bits = np.zeros((n, words * 64), dtype=np.uint8)
    flat = m.reshape(n, -1)
    bits[:, :flat.shape[1]] = flat
    return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int64).reshape(n, words))


class Case:
    """one (n, h, w, cin, cout) layer: inputs, packed weights, and the dense result per epilogue (computed once)"""

    def __init__(self, lib, gpu, n, h, w, cin, cout, outer, seed):
        from himo_amd.seflow.model import ConvDesc, ACT_SPLIT_IN
        self.lib, self.gpu, self.shape, self.outer = lib, gpu, (n, h, w, cin, cout), outer
        g = torch.Generator().manual_seed(seed)
        self.x = split_encode(torch.randn(n, h, w, cin, generator=g)).to(gpu)
        self.x0 = self.x.clone()
        self.wt = (0.1 * torch.randn(3, 3, cin, cout, generator=g)).to(gpu)
        self.bias = torch.randn(cout, generator=g).to(gpu)
        self.scale = (0.5 + torch.rand(cout, generator=g)).to(gpu)
        self.shift = (0.1 * torch.randn(cout, generator=g)).to(gpu)
        self.pk = torch.empty(int(lib.himo_conv_packed_weight_bytes(3, cin, cout)), dtype=torch.uint8, device=gpu)
        assert lib.himo_conv_pack_weights_ex(self.wt.data_ptr(), 3, cin, cout, 1, self.pk.data_ptr(), _stream()) == 0
        self.rows = (h + 7) // 8 * 8                     # mask rows per image: whole 8-row tiles, so bits past the image edge exist
        self.words = (self.rows * w + 63) // 64
        self.y = torch.empty((n, h, w, cout), dtype=torch.int32, device=gpu)
        self.dense = {}
        for epi in (EPI_BIAS, EPI_BIAS_BN_GELU):
            d = self.desc(epi, ACT_SPLIT_IN)
            d.tile_hint = 0x1008
            self.y.fill_(SENTINEL)
            assert lib.himo_conv2d(ctypes.byref(d), _stream()) == 0
            torch.cuda.synchronize()
            self.dense[epi] = self.y.clone()
            assert not bool((self.dense[epi] == SENTINEL).any())
        self.ConvDesc = ConvDesc

    def desc(self, epi, act, mask=None):
        from himo_amd.seflow.model import ConvDesc
        n, h, w, cin, cout = self.shape
        d = ConvDesc()
        d.x, d.x_pitch, d.w, d.bias = self.x.data_ptr(), cin, self.wt.data_ptr(), self.bias.data_ptr()
        d.scale, d.shift = self.scale.data_ptr(), self.shift.data_ptr()
        d.y, d.y_pitch = self.y.data_ptr(), cout
        d.h, d.w_in, d.cin, d.cout, d.ksize, d.stride, d.epilogue = h, w, cin, cout, 3, 1, epi
        d.w_packed, d.packed_format, d.act_layout = self.pk.data_ptr(), 1, act
        if self.outer:                                   # the n images as n samples of one frame each
            d.n, d.n_outer, d.x_outer_stride, d.y_outer_stride = 1, n, h * w * cin, h * w * cout
            d.x_batch_stride = d.y_batch_stride = 0
        else:
            d.n, d.x_batch_stride, d.y_batch_stride = n, h * w * cin, h * w * cout
        if mask is not None:
            d.mask = mask.data_ptr()
            d.mask_outer_stride, d.mask_batch_stride = (self.words, 0) if self.outer else (0, self.words)
        return d

    def masks(self):
        n, h, w, _, _ = self.shape
        rng = np.random.default_rng(1234)
        full = lambda: np.zeros((n, self.rows, w), dtype=bool)
        m = full(); m[:, :h] = True
        yield "all ones", m
        yield "all zeros", full()
        m = full(); m[:, :h] = rng.random((n, h, w)) < 0.37
        yield "37 % random", m
        tile_rows = min(8, h)
        for k in (1, 31, 32, 33, 256):
            if k > tile_rows * 32:
                continue
            m = full()
            pick = rng.permutation(tile_rows * 32)[:k]
            m[0, pick // 32, pick % 32] = True           # the first tile of the first image
            yield f"{k} pixels in one tile", m
        m = full(); m[:, [0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = True
        yield "four corners", m
        m = full(); m[:, h // 2, :] = True
        yield "one image row", m
        if self.rows > h:
            m = full(); m[:, h:] = True
            yield "only rows past the image edge", m


SHAPES = [(1, 8, 32, 64, 64, False), (1, 8, 32, 16, 64, False), (2, 19, 64, 64, 64, False), (2, 19, 64, 64, 64, True),
          (1, 64, 64, 128, 64, False), (1, 9, 32, 64, 32, False)]


@pytest.mark.parametrize("n,h,w,cin,cout,outer", SHAPES, ids=lambda v: str(v))
def test_masked_equals_dense_where_set_and_writes_nothing_else(lib, gpu, n, h, w, cin, cout, outer):
    from himo_amd.seflow.model import ACT_SPLIT_IN, ACT_ROW_MASK
    c = Case(lib, gpu, n, h, w, cin, cout, outer, seed=n * 1000 + h * 10 + cin)
    ran = 0
    for name, m in c.masks():
        mask = pack_mask(m, c.words).to(gpu)
        keep = torch.from_numpy(m[:, :h]).to(gpu)                     # [n][h][w]
        if name == "only rows past the image edge":
            assert not bool(keep.any()) and bool((mask != 0).any())
        for epi in (EPI_BIAS, EPI_BIAS_BN_GELU):
            c.y.fill_(SENTINEL)
            d = c.desc(epi, ACT_SPLIT_IN | ACT_ROW_MASK, mask)
            assert lib.himo_conv2d(ctypes.byref(d), _stream()) == 0, (name, epi)
            torch.cuda.synchronize()
            want = torch.where(keep[..., None], c.dense[epi], torch.full_like(c.y, SENTINEL))
            assert torch.equal(c.y, want), (name, epi, int((c.y != want).sum()))
            ran += 1
        assert torch.equal(c.x, c.x0), name
    assert ran >= 16


def test_refusals_write_nothing(lib, gpu):
    """include/himo_amd.h, HIMO_ACT_ROW_MASK: a NULL or misaligned mask is HIMO_ERR_INVALID_ARGUMENT, every other descriptor that
    carries the bit and is not admitted HIMO_ERR_UNSUPPORTED; nothing is written."""
    from himo_amd import _lib
    from himo_amd.seflow.model import ConvDesc, ACT_SPLIT_IN, ACT_ROW_MASK
    H = 8
    xb = torch.zeros(H * 64 * 128, dtype=torch.float32, device=gpu)
    wb = (0.1 * torch.randn(9 * 128 * 128)).to(gpu)
    bias = torch.zeros(128, device=gpu)
    y = torch.full((H * 64 * 128,), SENTINEL, dtype=torch.int32, device=gpu)
    mask = torch.full((64,), -1, dtype=torch.int64, device=gpu)
    packs = {}

    def packed(k, ci, co):
        if (k, ci, co) not in packs:
            p = torch.empty(int(lib.himo_conv_packed_weight_bytes(k, ci, co)), dtype=torch.uint8, device=gpu)
            assert lib.himo_conv_pack_weights_ex(wb.data_ptr(), k, ci, co, 1, p.data_ptr(), _stream()) == 0
            packs[(k, ci, co)] = p
        return packs[(k, ci, co)].data_ptr()

    def desc(k=3, stride=1, co=64, w=32, act=ACT_SPLIT_IN | ACT_ROW_MASK, mask_ptr=mask.data_ptr()):
        d = ConvDesc()
        d.x, d.x_batch_stride, d.x_pitch = xb.data_ptr(), H * w * 64, 64
        d.w, d.bias = wb.data_ptr(), bias.data_ptr()
        d.y, d.y_batch_stride, d.y_pitch = y.data_ptr(), H * w * co, co
        d.n, d.h, d.w_in, d.cin, d.cout, d.ksize, d.stride, d.epilogue = 1, H, w, 64, co, k, stride, 0
        d.w_packed, d.packed_format, d.act_layout = packed(k, 64, co), 1, act
        d.mask = mask_ptr
        return d

    table = {
        "stride 2": (desc(stride=2), _lib.ERR_UNSUPPORTED),
        "ksize 1": (desc(k=1), _lib.ERR_UNSUPPORTED),
        "cout 128": (desc(co=128), _lib.ERR_UNSUPPORTED),
        "w 48": (desc(w=48), _lib.ERR_UNSUPPORTED),
        "NULL mask": (desc(mask_ptr=None), _lib.ERR_INVALID_ARGUMENT),
        "misaligned mask": (desc(mask_ptr=mask.data_ptr() + 4), _lib.ERR_INVALID_ARGUMENT),
        "float32 input": (desc(act=ACT_ROW_MASK), _lib.ERR_UNSUPPORTED),
    }
    for name, (d, want) in table.items():
        st = lib.himo_conv2d(ctypes.byref(d), _stream())
        torch.cuda.synchronize()
        assert st == want, (name, st, want)
        assert bool(torch.all(y == SENTINEL)), f"{name}: refused but wrote"
    d = desc()                                           # the admitted form of the same descriptor does run
    assert lib.himo_conv2d(ctypes.byref(d), _stream()) == 0
    torch.cuda.synchronize()
    assert not bool((y[:H * 32 * 64] == SENTINEL).any())
