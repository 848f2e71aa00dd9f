// segiou.hip -- the downstream segmentation evaluator's confusion matrices (downstream/eval_seg.py:113-134, :248-265) for gfx950.
//
//   category uint8[T] + R prediction arrays uint8[T] + seg_valid uint8[T]  ->  int64 conf[R][2][3][3]  (+=)
//
// conf[r][mode][pred class][gt class], rows = prediction and columns = ground truth as iouEval.addBatch lays them out
// (eval_seg.py:126-134).  mode 0 counts every point (the reference as shipped: eval_seg.py:250 replaces the mask by ones),
// mode 1 the points whose seg_valid byte is non-zero (the reference with line 250 removed); the reference computes one of the
// two per run, here both leave the same pass.
//
// The class look-up table stands for the reference's three in-place assignments (eval_seg.py:255-257, :261-263):
//     x[~isin(x, CAR + OTHER_VEHICLES)] = 0;   x[isin(x, CAR)] = 1;   x[isin(x, OTHER_VEHICLES)] = 2
// Run one after the other on the SAME array they equal one table look-up only if no value written by a step is caught by a
// later one: step 1 writes 0 (NONE, in neither list), step 2 writes 1, step 3 writes 2.  With the AV2 indices 1 is ANIMAL, in
// neither list, so step 3 leaves the cars alone; 2 is ARTICULATED_BUS, in OTHER_VEHICLES, which step 3 maps to 2 again.  So
// lut[v] = 1 for REGULAR_VEHICLE, 2 for the nine OTHER_VEHICLES names, 0 otherwise, for every byte value (the host builds it
// from the package's category table; tests/test_eval_seg_cpu.py holds it against the reference's remap for 0..255).
//
// Traffic: (R + 2) bytes read per point, 144 R bytes of atomics per BLOCK, nothing else: 38 MB for 32 sweeps of 120 000 points
// with R = 8 -- bandwidth-trivial: a dozen microseconds at HBM rate, below what the launch's own bookkeeping costs (measured:
// 90 us at R = 8, 40 us at R = 2, about 0.4 TB/s; with one or two chunks per thread the 18 R shuffle reductions of the
// epilogue outweigh the counting -- profiles/eval_seg.txt; the program around it is bound by reading the files).  The sweeps of
// a packed batch need no offsets here: all arrays are packed alike and the matrices are sums over points, so the pass is flat.
//
// Work split: a thread takes 16 consecutive points per step as one 16-byte load per array (grid-stride over the T / 16 whole
// chunks).  Inside a chunk the nine bins of a (result, mode) are 6-bit fields of one 64-bit word (at most 16 per field per chunk),
// added as 1 << 6 (3 pred + gt), then spread over per-thread 32-bit register counters: no per-point atomics, no indexed
// register file.  The T % 16 points of the tail -- and everything when a base pointer is not 16-byte aligned -- go one
// point at a time through compare-and-add on the same counters, each point exactly once.  At the end: a shuffle reduction
// inside the wave, LDS across the block's four waves, one 64-bit global atomicAdd per non-zero bin per block.
#include "himo_common.h"
#include "blockops.h"

namespace himo {

constexpr int kSegThreads = 256;
constexpr int kSegWaves = kSegThreads / 64;
constexpr int kSegMaxBlocks = 1024;          // 4 per CU: enough loads in flight; bounds the atomics at 144 R x 1024
constexpr int kSegBins = 9;
constexpr int kSegField = 6;                 // bits per bin inside a chunk's packed word: 16 < 2^6

struct SegArgs {
    int64_t total;
    const uint8_t* gt;
    const uint8_t* valid;                    // may be nullptr: mode 1 then counts nothing
    const uint8_t* pred[HIMO_SEG_MAX_RESULTS];
    unsigned long long* conf;
    unsigned lut[64];                        // uint8[256]
};

__device__ inline unsigned byte_of(const uint4& v, int j) {
    const unsigned w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 255u;
}

template <int R, bool VEC>
__global__ __launch_bounds__(kSegThreads) void seg_confusion_kernel(const SegArgs a) {
    __shared__ unsigned s_lut[64];
    __shared__ unsigned s_part[kSegWaves][R * 2 * kSegBins];
    const int tid = threadIdx.x;
    if (tid < 64) s_lut[tid] = a.lut[tid];
    __syncthreads();
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(s_lut);

    unsigned cnt[R][2][kSegBins];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int b = 0; b < kSegBins; ++b) cnt[r][m][b] = 0;

    const int64_t gtid = (int64_t)blockIdx.x * kSegThreads + tid;
    const int64_t nthreads = (int64_t)gridDim.x * kSegThreads;
    const int64_t chunks = VEC ? a.total / 16 : 0;

    if (VEC) {
        for (int64_t c = gtid; c < chunks; c += nthreads) {
            const uint4 g4 = reinterpret_cast<const uint4*>(a.gt)[c];
            uint4 v4 = make_uint4(0, 0, 0, 0);
            if (a.valid) v4 = reinterpret_cast<const uint4*>(a.valid)[c];
            uint4 p4[R];
#pragma unroll
            for (int r = 0; r < R; ++r) p4[r] = reinterpret_cast<const uint4*>(a.pred[r])[c];
            unsigned gshift[16], msk[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                gshift[j] = kSegField * lut[byte_of(g4, j)];
                msk[j] = byte_of(v4, j) != 0 ? 1u : 0u;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                unsigned long long all = 0, masked = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const unsigned s = 3 * kSegField * lut[byte_of(p4[r], j)] + gshift[j];
                    all += 1ull << s;
                    masked += (unsigned long long)msk[j] << s;
                }
#pragma unroll
                for (int b = 0; b < kSegBins; ++b) {
                    cnt[r][0][b] += (unsigned)(all >> (kSegField * b)) & 63u;
                    cnt[r][1][b] += (unsigned)(masked >> (kSegField * b)) & 63u;
                }
            }
        }
    }
    for (int64_t i = chunks * 16 + gtid; i < a.total; i += nthreads) {
        const unsigned g = lut[a.gt[i]];
        const unsigned m = (a.valid && a.valid[i] != 0) ? 1u : 0u;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned code = 3 * lut[a.pred[r][i]] + g;
#pragma unroll
            for (int b = 0; b < kSegBins; ++b) {
                const unsigned hit = code == (unsigned)b ? 1u : 0u;
                cnt[r][0][b] += hit;
                cnt[r][1][b] += hit & m;
            }
        }
    }

    // wave -> block -> one atomic per bin.  A launch holds fewer than 2^31 points, so no partial sum leaves 32 bits.
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int b = 0; b < kSegBins; ++b) {
                const unsigned v = wave_sum(cnt[r][m][b]);
                if (lane == 0) s_part[wave][(r * 2 + m) * kSegBins + b] = v;
            }
    __syncthreads();
    if (tid < R * 2 * kSegBins) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < kSegWaves; ++w) sum += s_part[w][tid];
        if (sum != 0) atomicAdd(a.conf + tid, sum);
    }
}

template <int R>
static void launch_seg(const SegArgs& a, bool vec, hipStream_t s) {
    const int64_t work = vec ? a.total / 16 : a.total;
    int64_t blocks = (work + kSegThreads - 1) / kSegThreads;
    blocks = blocks < 1 ? 1 : blocks > kSegMaxBlocks ? kSegMaxBlocks : blocks;
    const dim3 grid((unsigned)blocks), block(kSegThreads);
    if (vec) hipLaunchKernelGGL((seg_confusion_kernel<R, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((seg_confusion_kernel<R, false>), grid, block, 0, s, a);
}

}  // namespace himo

using namespace himo;

extern "C" int himo_seg_confusion(int64_t total_points, const uint8_t* d_gt, const uint8_t* const* h_pred, int n_results,
                                  const uint8_t* d_seg_valid, const uint8_t* h_class_lut, int64_t* d_conf, void* stream) {
    if (total_points < 0 || total_points > (int64_t)0x7fffffff || n_results < 1 || n_results > HIMO_SEG_MAX_RESULTS ||
        !h_pred || !h_class_lut || !d_conf)
        return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points == 0) return HIMO_OK;
    if (!d_gt) return HIMO_ERR_INVALID_ARGUMENT;
    SegArgs a{};
    a.total = total_points;
    a.gt = d_gt;
    a.valid = d_seg_valid;
    a.conf = reinterpret_cast<unsigned long long*>(d_conf);
    bool vec = aligned16(d_gt) && aligned16(d_seg_valid);
    for (int r = 0; r < n_results; ++r) {
        if (!h_pred[r]) return HIMO_ERR_INVALID_ARGUMENT;
        a.pred[r] = h_pred[r];
        vec = vec && aligned16(h_pred[r]);
    }
    for (int k = 0; k < 256; ++k) {
        if (h_class_lut[k] > 2) return HIMO_ERR_INVALID_ARGUMENT;
        a.lut[k >> 2] |= (unsigned)h_class_lut[k] << (8 * (k & 3));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        ProfScope ps("seg_confusion_kernel", s);
        switch (n_results) {
            case 1: launch_seg<1>(a, vec, s); break;
            case 2: launch_seg<2>(a, vec, s); break;
            case 3: launch_seg<3>(a, vec, s); break;
            case 4: launch_seg<4>(a, vec, s); break;
            case 5: launch_seg<5>(a, vec, s); break;
            case 6: launch_seg<6>(a, vec, s); break;
            case 7: launch_seg<7>(a, vec, s); break;
            default: launch_seg<8>(a, vec, s); break;
        }
    }
    HIMO_LAUNCH_CHECK("seg_confusion_kernel");
    return HIMO_OK;
}
