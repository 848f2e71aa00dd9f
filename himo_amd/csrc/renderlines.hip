// renderlines.hip -- the headless viewer's line overlay ("line overlay, v1"; the rule is the module docstring of himo_amd/view.py) for
// gfx950.  The rule is this build's own: it is checked bit for bit against its numpy restatement (tests/renderlines_ref.py) and makes
// no claim about the pixels of any other viewer.
//
//   segments (float32 [n][6] = x0 y0 z0 x1 y1 z1) and a camera  ->  the lines buffer: one uint64 per pixel, ~0 = empty, else
//                                                                    (zq << 32) | segment index (himo_render_clear clears it)
//   the lines buffer (+ the point buffer, for the depth test)    ->  colours[idx] over an RGB image himo_render_resolve has written
//
// Two kernels:
//   render_lines_kernel      one wavefront per segment, four segments per 256-thread block.  Every lane redoes the float32 chain of
//                            rules A-C (camera coordinates, depth clip, projection, end pixels, end depths): a few dozen operations,
//                            cheaper than a broadcast and bit-identical on every lane.  The lanes then stride over the walk index k
//                            of rule D -- but only over a conservative k-interval computed in integers: a segment may be 2^21 pixels
//                            long with a sliver on screen, and no lane ever steps over off-screen pixels one by one.  Both screen
//                            coordinates are monotone in k, so each axis gives an interval by one floor division (exact along the
//                            major axis, where the coordinate is X0 +- k); the interval is widened by one at both ends and every
//                            pixel is tested.  The word is written as in the point splat: a plain load first, the 64-bit atomicMin
//                            only when the key is smaller.
//   render_composite_kernel  one pixel per lane: rule F.
//
// Built with -ffp-contract=off and without fast-math: every float operation rounds on its own, the divisions are the correctly rounded
// float32 division, as in numpy.  Everything after the end pixels is integer arithmetic (int64 where a product can pass 2^31).
#include "himo_common.h"
#include <math.h>

namespace himo {

constexpr int kRlThreads = 256;
constexpr int kRlWave = 64;
constexpr int kRlSegsPerBlock = kRlThreads / kRlWave;
constexpr unsigned long long kRlEmpty = ~0ull;
constexpr int kRlMaxSide = 16384;
constexpr float kRlScreenLimit = 1048576.0f;       // 2^20: |u|, |v| below it keep every product of rule D inside int64 (and 2 k dx inside 2^43)

__device__ inline long long rl_floordiv(long long a, long long b) {      // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// rule B for one end: (x, y, z) of the end, (ox, oy, oz) of the other, both ORIGINAL
__device__ inline void rl_clip_end(float x, float y, float z, float ox, float oy, float oz, float znear, float zfar, float& cx, float& cy,
                                   float& cz) {
    cx = x; cy = y; cz = z;
    if (z < znear || z > zfar) {
        const float plane = z < znear ? znear : zfar;
        const float t = (plane - z) / (oz - z);
        cx = x + t * (ox - x);
        cy = y + t * (oy - y);
        cz = plane;
    }
}

// rule D of the point splat
__device__ inline int rl_depth(float zc, const himo_camera& cam) {
    float t = zc - cam.znear;
    t = t * cam.inv_range;
    t = t * 16777216.0f;
    return (int)fminf(floorf(t), 16777215.0f);
}

// the k with lo <= C0 + floordiv(2 k d + steps, 2 steps) <= hi, as [kmin, kmax] widened by one at both ends (the caller tests every
// pixel); an empty interval comes back as kmin > kmax
__device__ inline void rl_axis_interval(long long c0, long long d, long long steps, long long lo, long long hi, long long& kmin,
                                        long long& kmax) {
    const long long a = lo - c0, b = hi - c0;                    // a <= c_k - C0 <= b
    if (d == 0) {
        if (a > 0 || b < 0) { kmin = 1; kmax = 0; }
        return;
    }
    const long long m = d > 0 ? d : -d;
    long long first, last;
    if (d > 0) {                                                 // non-decreasing in k
        first = rl_floordiv(2 * steps * a - steps, 2 * m);       //   2 k d + steps >= 2 steps a
        last = rl_floordiv(2 * steps * (b + 1) - steps, 2 * m);  //   2 k d + steps <  2 steps (b + 1)
    } else {                                                     // non-increasing in k
        first = rl_floordiv(steps - 2 * steps * (b + 1), 2 * m); //   2 k m > steps - 2 steps (b + 1)
        last = rl_floordiv(steps - 2 * steps * a, 2 * m);        //   2 k m <= steps - 2 steps a
    }
    first -= 1;
    last += 1;
    if (first > kmin) kmin = first;
    if (last < kmax) kmax = last;
}

__global__ __launch_bounds__(kRlThreads) void render_lines_kernel(int n, const float* __restrict__ seg, himo_camera cam, int half_px,
                                                                   uint32_t index_base, unsigned long long* __restrict__ lines) {
    const int lane = threadIdx.x & (kRlWave - 1);
    const int i = blockIdx.x * kRlSegsPerBlock + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* q = seg + (int64_t)i * 6;
    const float ax = q[0], ay = q[1], az = q[2], bx = q[3], by = q[4], bz = q[5];
    // A. camera coordinates of both ends
    const float* m = cam.m;
    const float xa = ((m[0] * ax + m[1] * ay) + m[2] * az) + m[3];
    const float ya = ((m[4] * ax + m[5] * ay) + m[6] * az) + m[7];
    const float za = ((m[8] * ax + m[9] * ay) + m[10] * az) + m[11];
    const float xb = ((m[0] * bx + m[1] * by) + m[2] * bz) + m[3];
    const float yb = ((m[4] * bx + m[5] * by) + m[6] * bz) + m[7];
    const float zb = ((m[8] * bx + m[9] * by) + m[10] * bz) + m[11];
    if (!isfinite(xa) || !isfinite(ya) || !isfinite(za) || !isfinite(xb) || !isfinite(yb) || !isfinite(zb)) return;
    // B. depth clip, both ends from the original pair
    if ((za < cam.znear && zb < cam.znear) || (za > cam.zfar && zb > cam.zfar)) return;
    float pxa, pya, pza, pxb, pyb, pzb;
    rl_clip_end(xa, ya, za, xb, yb, zb, cam.znear, cam.zfar, pxa, pya, pza);
    rl_clip_end(xb, yb, zb, xa, ya, za, cam.znear, cam.zfar, pxb, pyb, pzb);
    // C. screen
    float u0, v0, u1, v1;
    if (cam.ortho) {
        u0 = cam.fx * pxa + cam.cx; v0 = cam.fy * pya + cam.cy;
        u1 = cam.fx * pxb + cam.cx; v1 = cam.fy * pyb + cam.cy;
    } else {
        u0 = cam.fx * (pxa / pza) + cam.cx; v0 = cam.fy * (pya / pza) + cam.cy;
        u1 = cam.fx * (pxb / pzb) + cam.cx; v1 = cam.fy * (pyb / pzb) + cam.cy;
    }
    if (!isfinite(u0) || !isfinite(v0) || !isfinite(u1) || !isfinite(v1)) return;
    if (fabsf(u0) >= kRlScreenLimit || fabsf(v0) >= kRlScreenLimit || fabsf(u1) >= kRlScreenLimit || fabsf(v1) >= kRlScreenLimit) return;
    const int X0 = (int)floorf(u0), Y0 = (int)floorf(v0), X1 = (int)floorf(u1), Y1 = (int)floorf(v1);
    const int zq0 = rl_depth(pza, cam), zq1 = rl_depth(pzb, cam);
    // D. the walk, over the k whose pixel's disc can reach the image
    const long long dx = X1 - X0, dy = Y1 - Y0, dz = zq1 - zq0;
    const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const long long steps = adx > ady ? adx : ady;
    const unsigned long long low = (unsigned long long)(index_base + (uint32_t)i);
    const int r2 = half_px * half_px;
    long long kmin = 0, kmax = steps;
    if (steps == 0) {
        if (X0 < -half_px || X0 > cam.width - 1 + half_px || Y0 < -half_px || Y0 > cam.height - 1 + half_px) return;
    } else {
        rl_axis_interval(X0, dx, steps, -half_px, (long long)cam.width - 1 + half_px, kmin, kmax);
        rl_axis_interval(Y0, dy, steps, -half_px, (long long)cam.height - 1 + half_px, kmin, kmax);
    }
    for (long long k = kmin + lane; k <= kmax; k += kRlWave) {
        int x = X0, y = Y0, zq = zq0;
        if (steps != 0) {
            x = X0 + (int)rl_floordiv(2 * k * dx + steps, 2 * steps);
            y = Y0 + (int)rl_floordiv(2 * k * dy + steps, 2 * steps);
            zq = zq0 + (int)rl_floordiv(k * dz, steps);
        }
        // E. the 64-bit minimum into the disc
        const unsigned long long key = ((unsigned long long)(uint32_t)zq << 32) | low;
        for (int ddy = -half_px; ddy <= half_px; ++ddy) {
            const int qy = y + ddy;
            if (qy < 0 || qy >= cam.height) continue;
            for (int ddx = -half_px; ddx <= half_px; ++ddx) {
                const int qx = x + ddx;
                if (ddx * ddx + ddy * ddy > r2 || qx < 0 || qx >= cam.width) continue;
                unsigned long long* w = lines + (qy * cam.width + qx);
                if (*w > key) atomicMin(w, key);
            }
        }
    }
}

__global__ __launch_bounds__(kRlThreads) void render_composite_kernel(const unsigned long long* __restrict__ lines,
                                                                       const unsigned long long* __restrict__ vis, int cells,
                                                                       const uint32_t* __restrict__ colors, int64_t n_colors, uint32_t neutral,
                                                                       unsigned char* __restrict__ rgb) {
    const int p = blockIdx.x * kRlThreads + threadIdx.x;
    if (p >= cells) return;
    const unsigned long long key = lines[p];
    if (key == kRlEmpty) return;
    if (vis) {
        const unsigned long long pt = vis[p];
        if (pt != kRlEmpty && (uint32_t)(pt >> 32) < (uint32_t)(key >> 32)) return;      // a nearer point hides the line; a tie shows it
    }
    const uint32_t idx = (uint32_t)key;
    const uint32_t c = (int64_t)idx < n_colors ? colors[idx] : neutral;
    unsigned char* out = rgb + (int64_t)p * 3;
    out[0] = (unsigned char)(c & 0xFFu); out[1] = (unsigned char)((c >> 8) & 0xFFu); out[2] = (unsigned char)((c >> 16) & 0xFFu);
}

}  // namespace himo

using namespace himo;

extern "C" int himo_render_lines(int64_t n, const float* d_seg, const himo_camera* cam, int half_px, uint32_t index_base,
                                 uint64_t* d_lines, void* stream) {
    if (n < 0 || half_px < 0 || half_px > 3 || !cam || cam->width <= 0 || cam->height <= 0) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_lines || (reinterpret_cast<uintptr_t>(d_lines) & 7u) || (n > 0 && !d_seg) || (reinterpret_cast<uintptr_t>(d_seg) & 3u))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (!isfinite(cam->znear) || !isfinite(cam->zfar) || !(cam->zfar > cam->znear) || !isfinite(cam->inv_range) || !(cam->inv_range > 0.f))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (cam->width > kRlMaxSide || cam->height > kRlMaxSide || n > 0x7fffffffLL || (int64_t)index_base + n > 0x100000000LL)
        return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("render_lines_kernel", s);
        hipLaunchKernelGGL(render_lines_kernel, dim3((unsigned)((n + kRlSegsPerBlock - 1) / kRlSegsPerBlock)), dim3(kRlThreads), 0, s, (int)n,
                           d_seg, *cam, half_px, index_base, reinterpret_cast<unsigned long long*>(d_lines));
    }
    HIMO_LAUNCH_CHECK("render_lines_kernel");
    return HIMO_OK;
}

extern "C" int himo_render_composite(const uint64_t* d_lines, const uint64_t* d_vis, int width, int height, const uint32_t* d_colors,
                                     int64_t n_colors, uint32_t neutral, unsigned char* d_rgb, void* stream) {
    if (width <= 0 || height <= 0 || !d_lines || (reinterpret_cast<uintptr_t>(d_lines) & 7u) || (reinterpret_cast<uintptr_t>(d_vis) & 7u) || !d_rgb)
        return HIMO_ERR_INVALID_ARGUMENT;
    if (n_colors < 0 || (n_colors > 0 && !d_colors) || (reinterpret_cast<uintptr_t>(d_colors) & 3u)) return HIMO_ERR_INVALID_ARGUMENT;
    if (width > kRlMaxSide || height > kRlMaxSide) return HIMO_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int cells = width * height;
    {
        ProfScope ps("render_composite_kernel", s);
        hipLaunchKernelGGL(render_composite_kernel, dim3((unsigned)((cells + kRlThreads - 1) / kRlThreads)), dim3(kRlThreads), 0, s,
                           reinterpret_cast<const unsigned long long*>(d_lines), reinterpret_cast<const unsigned long long*>(d_vis), cells,
                           d_colors, n_colors, neutral, d_rgb);
    }
    HIMO_LAUNCH_CHECK("render_composite_kernel");
    return HIMO_OK;
}
