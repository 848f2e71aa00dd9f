// conv_plan.h -- the ONE place that decides a himo_conv2d call (host code only): descriptor validation, the act_layout
// admissibility table, which of the five kernel families answers, its tile (heuristic or tile_hint), grid, 16-byte store
// path and profiler name.  plan_conv reads nothing but the descriptor; the kernel files only map a finished plan to a
// template instantiation (launch_conv_*).  The table of tile_hint values in include/himo_amd.h is taken from here.
#pragma once
#include "conv_common.h"

namespace himo {

enum ConvFamily {
    kConvF32,         // conv.hip: float32 MFMA -- no w_packed; 3x3 stride 2 with a GRU epilogue or a plain tile hint
    kConvStaged,      // convbf.hip: split precision, weights through LDS -- row GEMMs / 1x1; 3x3 stride 1 that kConvFromL2 declines or a plain hint pins
    kConvFromL2,      // convsp.hip: split precision, weights from L2 -- 3x3 on float32 maps (stride 1 | 2, plain epilogues)
    kConvPresplit3,   // convsg.hip: input in the split activation format (HIMO_ACT_SPLIT_IN), LDS-DMA -- 3x3
    kConvPresplit1    // ... 1x1
};

struct ConvPlan {
    ConvFamily family;
    ConvArgs args;              // final: act_flags already carries kActVecStore where the family stores 16 bytes at a time
    int ks, stride, epi, fmt;   // fmt = himo_conv_desc.packed_format (unused by kConvF32)
    int bn, mi, ph, nt;         // the template parameters the family's ladder switches on (bn: channels per block)
    const void* w_packed;
    dim3 grid;
    const char* prof_name;      // ProfScope family name: bench.py --full and the scripts/ summaries key on it
};

void launch_conv_f32(const ConvPlan& p, hipStream_t s);         // conv.hip
void launch_conv_staged(const ConvPlan& p, hipStream_t s);      // convbf.hip
void launch_conv_from_l2(const ConvPlan& p, hipStream_t s);     // convsp.hip
void launch_conv_presplit3(const ConvPlan& p, hipStream_t s);   // convsg.hip
void launch_conv_presplit1(const ConvPlan& p, hipStream_t s);   // convsg.hip

// blocks of a launch: tiles of th x tw output pixels (th = 0: tw consecutive rows of a row GEMM) x bn channels
inline int64_t blocks_for(const ConvArgs& a, int th, int tw, int bn) {
    const int64_t tiles = th ? (int64_t)((a.Ho + th - 1) / th) * ((a.Wo + tw - 1) / tw) : ((int64_t)a.Ho * a.Wo + tw - 1) / tw;
    return (int64_t)a.N * tiles * ((a.Cout + bn - 1) / bn);
}

// one image of `pixels` x `pitch` floats stays below 2 GB: 32-bit byte offsets into it (buffer resources, DMA sources)
inline bool below_2gb(int64_t pixels, int pitch) { return pixels * pitch * 4 < ((int64_t)1 << 31); }

// "conv" (1x1 | 3x3 | 3x3s2) "_" (mfma | bf16x3 | f16x2 | bf16x2) "_kernel"; fmt < 0 = float32
inline const char* conv_prof_name(int ks, int stride, int fmt) {
    static const char* const names[3][4] = {
        {"conv1x1_mfma_kernel", "conv1x1_bf16x3_kernel", "conv1x1_f16x2_kernel", "conv1x1_bf16x2_kernel"},
        {"conv3x3_mfma_kernel", "conv3x3_bf16x3_kernel", "conv3x3_f16x2_kernel", "conv3x3_bf16x2_kernel"},
        {"conv3x3s2_mfma_kernel", "conv3x3s2_bf16x3_kernel", "conv3x3s2_f16x2_kernel", "conv3x3s2_bf16x2_kernel"}};
    return names[ks == 1 ? 0 : stride == 2 ? 2 : 1][fmt < 0 ? 0 : fmt == 1 ? 2 : fmt == 2 ? 3 : 1];
}

// The two LDS-staged structures (kConvF32: rows_per_mi 4, tw 16; kConvStaged: 2, 32): a block is 64 * mi pixels
// (rows_per_mi * mi image rows x tw columns of a 3x3 layer) x bn channels.  128 x 128 when that still gives two blocks
// per CU, else shrink M, then N (keep128: the z|r split of the float32 GRU epilogue needs the 128-wide channel tile).
// hint (bn << 4) | mi pins the tile; a malformed one, or 128 where Cout is no multiple of 128, is ignored.
inline void plan_staged_tile(ConvPlan& p, int rows_per_mi, int tw, bool keep128, int hint) {
    const ConvArgs& a = p.args;
    auto blocks = [&](int bn, int mi) { return p.ks == 1 ? blocks_for(a, 0, 64 * mi, bn) : blocks_for(a, rows_per_mi * mi, tw, bn); };
    const bool can128 = a.Cout >= 128 && (a.Cout % 128) == 0;
    int bn = can128 ? 128 : 64, mi = 2;
    if (blocks(bn, mi) < 512) mi = 1;
    if (blocks(bn, mi) < 512 && bn == 128 && !keep128) bn = 64;
    const int hb = hint >> 4, hm = hint & 15;
    if ((hb == 64 || (hb == 128 && can128)) && (hm == 1 || hm == 2)) { bn = hb; mi = hm; }
    p.bn = bn; p.mi = mi;
    p.grid = dim3((unsigned)blocks(bn, mi));
}

// The weights-from-L2 and LDS-DMA structures: a wave owns mi x ph image rows (32-pixel segments of a row GEMM) of 32
// pixels, the block's four waves 4 / ph pixel groups x nt 32-channel column tiles each
inline void plan_rows_tile(ConvPlan& p, int ph, int mi, int nt) {
    p.ph = ph; p.mi = mi; p.nt = nt; p.bn = (4 / ph) * 32 * nt;
    p.grid = dim3((unsigned)(p.ks == 1 ? blocks_for(p.args, 0, mi * ph * 32, p.bn) : blocks_for(p.args, mi * ph, 32, p.bn)));
}

// kConvFromL2: 3x3 layers (stride 1 | 2) on float32 maps with a plain epilogue.  false = this structure declines the
// call and nothing of p has changed.  rows_hint (tile_hint & 15): 0 = heuristic; 4 | 2 | 1 image rows per wave (stride 2:
// 2 | 1); stride 1, two-term formats: 5 | 6 = 64-channel blocks forced (wide layers too), 1 | 2 rows per wave; 9 | 10 =
// four pixel groups x one 32-channel tile, 1 | 2 rows per wave.
inline bool plan_from_l2(ConvPlan& p, int rows_hint) {
    ConvArgs& a = p.args;
    const bool vec = vec_store_ok(a);
    if (p.epi == kEpiGruZR || p.epi == kEpiGruQ) return false;
    if (p.fmt == 2 && (p.epi != kEpiBias || (a.act_flags & ~(kActAccumulate | kActStuffedIn)))) return false;   // two-term bf16: float32 maps, bias epilogue
    if ((a.act_flags & kActAccumulate) && (p.fmt != 2 || !vec)) return false;              // y += result: that kernel's 16-byte store path only
    if ((a.act_flags & kActStuffedIn) && (p.fmt != 2 || p.stride != 1)) return false;      // zero-stuffed input: that kernel, stride 1
    if (!below_2gb((int64_t)a.H * a.W, a.x_pitch)) return false;
    const bool ph_ok = p.stride == 1 && p.fmt != 0;
    const int ph_hint = (ph_ok && (rows_hint == 5 || rows_hint == 6)) ? 2 : (ph_ok && (rows_hint == 9 || rows_hint == 10)) ? 4 : 0;
    if (!ph_hint && rows_hint > 4) return false;
    const bool wide = a.Cout > 64 && ph_hint == 0;     // PH = 1: 128-channel tiles; PH = 2: 64-channel tiles
    const int ph = ph_hint ? ph_hint : (wide ? 1 : 2);
    int mi = blocks_for(a, 4 * ph, 32, (4 / ph) * 32) >= 1024 ? 4 : 2;            // two blocks per CU, at least two rounds of them
    if (rows_hint == 4 || rows_hint == 2 || rows_hint == 1) mi = rows_hint;
    if (ph_hint) mi = rows_hint & 3;
    if (p.stride == 2) mi = (rows_hint == 1 || rows_hint == 2) ? rows_hint : (wide ? 2 : 1);   // (64-channel blocks: keeps the 5 x 65 patch double-buffered)
    p.family = kConvFromL2;
    plan_rows_tile(p, ph, mi, 1);
    p.prof_name = conv_prof_name(3, p.stride, p.fmt);
    if (vec && (!(a.act_flags & kActSplitOut) || !(a.Cout & 15))) a.act_flags |= kActVecStore;
    return true;
}

// kConvPresplit1 | kConvPresplit3: input in the split activation format (fp16-split weights, bias or bias + BN + GELU,
// whole 16-channel groups: the act_layout table of plan_conv has checked).
// rows_hint: 4 | 2 | 1 = 32-pixel segments (1x1) / image rows (3x3 stride 1) per wave, 4 on 64-channel layers becomes 2;
// 8 (64-channel layers) | 12 (wide layers) = two 32-channel column tiles per wave, only with a 16-byte-storable output;
// anything else, and every hint at stride 2 (one variant per width class), leaves the heuristic in charge.
// kActRowMask (admitted by plan_conv's table): ONE variant -- the 8-row x 32-pixel x 64-channel tile of rows_hint 8 whose
// fragments are the tile's listed pixels (conv3_rowmask_kernel) -- under a profiler name of its own; every hint is ignored.
inline int plan_presplit(ConvPlan& p, int rows_hint) {
    ConvArgs& a = p.args;
    if (!below_2gb((int64_t)a.H * a.W, a.x_pitch)) return HIMO_ERR_UNSUPPORTED;       // 32-bit DMA source offsets
    if (a.act_flags & kActRowMask) {
        p.family = kConvPresplit3;
        p.prof_name = "conv3x3_masked_f16x2_kernel";
        plan_rows_tile(p, 4, 2, 2);
        return HIMO_OK;
    }
    const bool wide = a.Cout > 64, vec = vec_store_ok(a), pinned = rows_hint == 4 || rows_hint == 2 || rows_hint == 1;
    const int ph = wide ? 1 : 2;
    p.family = p.ks == 1 ? kConvPresplit1 : kConvPresplit3;
    p.prof_name = conv_prof_name(p.ks, p.stride, 1);
    if (vec) a.act_flags |= kActVecStore;
    if (p.ks == 1) {
        int mi = wide ? 4 : 2;
        while (mi > 1 && blocks_for(a, 0, mi * ph * 32, (4 / ph) * 32) < 2048) mi >>= 1;
        if (pinned) mi = rows_hint;
        plan_rows_tile(p, ph, !wide && mi == 4 ? 2 : mi, 1);
    } else if (p.stride == 2) {                         // two output rows per block: a 5-row x 80-slot patch, double-buffered
        plan_rows_tile(p, ph, wide ? 2 : 1, 1);
    } else if (!wide && rows_hint == 8 && vec) {
        // a wave owns 2 rows x 32 pixels x BOTH 32-channel column tiles (every activation fragment meets two weight fragments),
        // four waves = an 8-row tile on a 10-row patch (1.25x halo instead of 1.5x; 51 KB: three blocks per CU)
        plan_rows_tile(p, 4, 2, 2);
    } else if (wide && rows_hint == 12 && vec) {
        // 4 rows x 64 channels per wave (128 accumulator registers, two waves per SIMD): half the fragment reads AND half the
        // weight loads per matrix instruction; 3-4 % on the 256-channel decoder layers, slower on the 128-channel encoder
        // ones (the autotune decides per layer)
        plan_rows_tile(p, a.Cout % 256 == 0 ? 1 : 2, 4, 2);
    } else {
        int mi = blocks_for(a, 4 * ph, 32, (4 / ph) * 32) >= 1024 ? 4 : 2;
        if (pinned) mi = rows_hint;
        plan_rows_tile(p, ph, !wide && mi == 4 ? 2 : mi, 1);   // 64-channel blocks: 8-row patches would not leave three blocks per CU
    }
    return HIMO_OK;
}

inline int plan_conv(const himo_conv_desc& d, ConvPlan& p) {
    if (!d.x || !d.w || !d.y) return HIMO_ERR_INVALID_ARGUMENT;
    if (d.n < 1 || d.h < 1 || d.w_in < 1 || d.cin < 1 || d.cout < 1) return HIMO_ERR_INVALID_ARGUMENT;
    if (!(d.ksize == 1 || d.ksize == 3) || !(d.stride == 1 || d.stride == 2)) return HIMO_ERR_UNSUPPORTED;
    if (d.ksize == 1 && d.stride != 1) return HIMO_ERR_UNSUPPORTED;
    if (d.epilogue < 0 || d.epilogue > kEpiReluMask) return HIMO_ERR_INVALID_ARGUMENT;
    if (d.epilogue == kEpiBiasBnGelu && (!d.scale || !d.shift)) return HIMO_ERR_INVALID_ARGUMENT;
    const bool gru = d.epilogue == kEpiGruZR || d.epilogue == kEpiGruQ;
    if (gru && (!d.aux_in || !d.aux_out)) return HIMO_ERR_INVALID_ARGUMENT;
    if (d.epilogue == kEpiReluMask && !d.aux_in) return HIMO_ERR_INVALID_ARGUMENT;
    // 16-byte vector loads: channel counts / pitches / bases must be multiples of 4 floats
    if ((d.cin & 3) || (d.cout & 3) || (d.x_pitch & 3) || (d.x_batch_stride & 3) || !aligned16(d.x) || !aligned16(d.w))
        return HIMO_ERR_UNSUPPORTED;
    const int n_outer = d.n_outer > 1 ? d.n_outer : 1;
    if (n_outer > 1 && ((d.x_outer_stride & 3) || (d.y_outer_stride & 3))) return HIMO_ERR_INVALID_ARGUMENT;
    p = ConvPlan{};
    p.ks = d.ksize; p.stride = d.stride; p.epi = d.epilogue; p.fmt = d.packed_format; p.w_packed = d.w_packed;
    ConvArgs& a = p.args;
    a.x = d.x; a.x_batch_stride = d.x_batch_stride; a.x_pitch = d.x_pitch;
    a.w = d.w; a.bias = d.bias; a.scale = d.scale; a.shift = d.shift;
    a.y = d.y; a.y_batch_stride = d.y_batch_stride; a.y_pitch = d.y_pitch;
    a.N = d.n * n_outer; a.n_inner = d.n; a.x_outer_stride = d.x_outer_stride; a.y_outer_stride = d.y_outer_stride;
    a.H = d.h; a.W = d.w_in; a.Cin = d.cin; a.Cout = d.cout;
    a.Ho = d.stride == 2 ? (d.h + 1) / 2 : d.h;      // 3x3, pad 1: ceil(H / stride)
    a.Wo = d.stride == 2 ? (d.w_in + 1) / 2 : d.w_in;
    a.aux_in = d.aux_in; a.aux_in_pitch = d.aux_in_pitch; a.aux_out = d.aux_out; a.aux_out_pitch = d.aux_out_pitch;
    a.act_flags = d.act_layout;
    a.range_seen = (d.act_layout & kActSplitOut) ? d.d_range_seen : nullptr;

    // ---- act_layout: which combinations exist at all ----
    // HIMO_ACT_ROW_MASK: the split-input fp16-split 3x3 stride-1 layers of <= 64 channels with a float32 output, whole 32-pixel
    // row segments (a tile row's 32 mask bits are one aligned 32-bit word); the mask is read by plan_presplit's kernel only
    if (d.act_layout & kActRowMask) {
        if (!d.d_mask || (reinterpret_cast<uintptr_t>(d.d_mask) & 7u)) return HIMO_ERR_INVALID_ARGUMENT;
        if (d.act_layout != (kActRowMask | kActSplitIn) || !d.w_packed || d.packed_format != 1 || d.ksize != 3 || d.stride != 1 ||
            d.cout > 64 || (d.w_in & 31) || (d.epilogue != kEpiBias && d.epilogue != kEpiBiasBnGelu) || (d.cin & 15) || (d.x_pitch & 15))
            return HIMO_ERR_UNSUPPORTED;
        a.mask = reinterpret_cast<const unsigned long long*>(d.d_mask);
        a.mask_batch_stride = d.mask_batch_stride; a.mask_outer_stride = d.mask_outer_stride;
    }
    // HIMO_ACT_ACCUMULATE alone on a row GEMM (ksize 1) of either bf16 split with the bias epilogue: kConvStaged
    const bool gemm_acc = d.act_layout == kActAccumulate && d.w_packed && d.ksize == 1 && d.epilogue == kEpiBias && (d.packed_format == 0 || d.packed_format == 2);
    if (d.act_layout & (kActAccumulate | kActStuffedIn)) {
        // otherwise y += result / the compact input read zero-stuffed: the two-term bf16 3x3 stride-1 kernel with the bias epilogue only
        if (!gemm_acc && ((d.act_layout & ~(kActAccumulate | kActStuffedIn)) || !d.w_packed || d.packed_format != 2 || d.ksize != 3 ||
                          d.stride != 1 || d.epilogue != kEpiBias))
            return HIMO_ERR_UNSUPPORTED;
        if ((d.act_layout & kActStuffedIn) && ((d.h & 1) || (d.w_in & 1) || !below_2gb((int64_t)(d.h / 2) * (d.w_in / 2), d.x_pitch)))
            return HIMO_ERR_UNSUPPORTED;
    } else if (d.act_layout && !(d.act_layout & kActRowMask)) {   // split activation format: fp16-split layers only, whole 16-channel groups
        if ((d.act_layout & ~(kActSplitIn | kActSplitOut)) || !d.w_packed || d.packed_format != 1) return HIMO_ERR_UNSUPPORTED;
        if (d.ksize == 1 && !(d.act_layout & kActSplitIn)) return HIMO_ERR_UNSUPPORTED;      // 1x1: split output only with split input
        if (d.epilogue != kEpiBias && d.epilogue != kEpiBiasBnGelu) return HIMO_ERR_UNSUPPORTED;
        if (((d.act_layout & kActSplitIn) && ((d.cin & 15) || (d.x_pitch & 15))) ||
            ((d.act_layout & kActSplitOut) && ((d.cout & 15) || (d.y_pitch & 15))))
            return HIMO_ERR_UNSUPPORTED;
    }

    // ---- float32: no packed weights, and the 3x3 stride-2 layers with a GRU epilogue or a pinned plain tile ----
    const int hint = d.tile_hint, rows_hint = hint & 15;
    const bool l2_hint = hint == 0 || (hint & 0x1000);
    if (!d.w_packed || (d.stride == 2 && (gru || !l2_hint))) {
        p.family = kConvF32;
        plan_staged_tile(p, 4, 16, d.epilogue == kEpiGruZR, hint);
        p.prof_name = conv_prof_name(d.ksize, d.stride, -1);
        // row GEMMs: 16-byte epilogue stores when the output (and, for the ReLU-mask epilogue, the mask source) admits them
        if (d.ksize == 1 && vec_store_ok(a) && !(a.Cout & 31) && (d.epilogue != kEpiReluMask || (aligned16(a.aux_in) && !(a.aux_in_pitch & 3))))
            a.act_flags |= kActVecStore;
        return HIMO_OK;
    }
    // ---- split precision ----
    if (a.act_flags & kActSplitIn) return plan_presplit(p, rows_hint);
    // (the row GEMMs' 32-bit-offset epilogue is the one that implements y += result)
    const bool gemm_accumulate = gemm_acc && (int64_t)a.Ho * a.Wo * a.y_pitch < (1ll << 30);
    // 3x3 layers: the weights-from-L2 structure (0x1000 | rows_hint pins its variant) unless the caller pins a tile of the
    // LDS-staged kernel; stride 2 arrives here with such a hint only
    const bool from_l2 = d.ksize == 3 && l2_hint;
    if (a.act_flags && !gemm_accumulate && !from_l2) return HIMO_ERR_UNSUPPORTED;
    if (from_l2 && plan_from_l2(p, rows_hint)) return HIMO_OK;
    if (d.ksize == 3 && (hint & 0x1000) && rows_hint > 4) return HIMO_ERR_UNSUPPORTED;     // a pinned variant this layer does not admit
    if (d.stride != 1) return HIMO_ERR_UNSUPPORTED;
    if (!below_2gb((int64_t)a.H * a.W, a.x_pitch)) return HIMO_ERR_UNSUPPORTED;
    // two-term bf16: 3x3 in kConvFromL2 only, row GEMMs here
    if (d.packed_format == 2 && (d.ksize != 1 || (d.epilogue != kEpiBias && d.epilogue != kEpiReluMask) || (a.act_flags && !gemm_accumulate)))
        return HIMO_ERR_UNSUPPORTED;
    p.family = kConvStaged;                              // (never sets kActVecStore: this kernel has no 16-byte store path)
    plan_staged_tile(p, 2, 32, false, hint);
    p.prof_name = conv_prof_name(d.ksize, 1, d.packed_format);
    return HIMO_OK;
}

}  // namespace himo
