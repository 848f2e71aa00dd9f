// render.hip -- the headless viewer's renderer ("point splat, v1"; the rule is the module docstring of himo_amd/view.py) for gfx950.
// The rule is this build's own: it is checked bit for bit against its numpy restatement (tests/render_ref.py) and makes no claim
// about the pixels of any other viewer.
//
//   points (+ a per-point offset, + a skip byte) and a camera  ->  the visibility buffer: one uint64 per pixel,
//                                                                  ~0 = empty, else (zq << 32) | point index
//   the visibility buffer and per-point attributes             ->  uint8 RGB [height][width][3]
//
// Three kernels:
//   render_clear_kernel    fills the buffer with ~0.
//   render_splat_kernel    one point per lane, 256-thread blocks: offset add, world -> camera, projection, the 24-bit depth, then a
//                          64-bit atomicMin of the key into every pixel of the disc that lies inside the image.  The nearest point
//                          wins, the lowest index among equal depths, so the buffer is a pure function of the set of (point, index):
//                          launch order and the split over calls cannot change a bit.  The pixel word is read with a plain load
//                          first and the atomic issued only when the key is smaller: words only ever decrease, so a stale read
//                          costs a redundant atomic, never a wrong buffer.  Plain global atomics, no tile binning (v1).
//   render_resolve_kernel  one pixel per lane: the colour of the point under it (three modes), eye-dome shading from the depths of
//                          the four neighbours at +-edl_px, three bytes out.
//
// Built with -ffp-contract=off and without fast-math: every float operation rounds on its own, the perspective divide is the
// correctly rounded float32 division, as in numpy.
#include "himo_common.h"
#include <math.h>

namespace himo {

constexpr int kRdThreads = 256;
constexpr unsigned long long kRdEmpty = ~0ull;
constexpr int kRdMaxSide = 16384;            // width + radius + 1 stays exact in float32, width * height far inside int32

__global__ __launch_bounds__(kRdThreads) void render_clear_kernel(unsigned long long* __restrict__ vis, int cells) {
    const int i = blockIdx.x * kRdThreads + threadIdx.x;
    if (i < cells) vis[i] = kRdEmpty;
}

__global__ __launch_bounds__(kRdThreads) void render_splat_kernel(int n, const float* __restrict__ pts, int pitch,
                                                                   const float* __restrict__ offset, const unsigned char* __restrict__ skip,
                                                                   himo_camera cam, int radius, uint32_t index_base,
                                                                   unsigned long long* __restrict__ vis) {
    const int i = blockIdx.x * kRdThreads + threadIdx.x;
    if (i >= n) return;
    if (skip && skip[i]) return;
    const float* q = pts + (int64_t)i * pitch;
    float x = q[0], y = q[1], z = q[2];
    if (offset) {
        const float* o = offset + (int64_t)i * 3;
        x = x + o[0]; y = y + o[1]; z = z + o[2];
    }
    const float* m = cam.m;
    const float xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    if (!isfinite(xc) || !isfinite(yc) || !isfinite(zc) || zc < cam.znear || zc > cam.zfar) return;
    float u, v;
    if (cam.ortho) {
        u = cam.fx * xc + cam.cx;
        v = cam.fy * yc + cam.cy;
    } else {
        u = cam.fx * (xc / zc) + cam.cx;
        v = cam.fy * (yc / zc) + cam.cy;
    }
    if (!isfinite(u) || !isfinite(v)) return;
    const float lo = -(float)(radius + 1);
    if (u < lo || !(u < (float)(cam.width + radius + 1)) || v < lo || !(v < (float)(cam.height + radius + 1))) return;    // in float,
    const int px = (int)floorf(u), py = (int)floorf(v);                                               // before any conversion to int
    float t = zc - cam.znear;
    t = t * cam.inv_range;
    t = t * 16777216.0f;
    const uint32_t zq = (uint32_t)fminf(floorf(t), 16777215.0f);                                      // (t >= 0: zc >= znear)
    const unsigned long long key = ((unsigned long long)zq << 32) | (unsigned long long)(index_base + (uint32_t)i);
    const int r2 = radius * radius;
    for (int dy = -radius; dy <= radius; ++dy) {
        const int qy = py + dy;
        if (qy < 0 || qy >= cam.height) continue;
        for (int dx = -radius; dx <= radius; ++dx) {
            const int qx = px + dx;
            if (dx * dx + dy * dy > r2 || qx < 0 || qx >= cam.width) continue;
            unsigned long long* w = vis + (qy * cam.width + qx);
            if (*w > key) atomicMin(w, key);
        }
    }
}

__device__ inline float rd_depth_log(unsigned long long key) {
    return key == kRdEmpty ? 24.0f : log2f((float)((uint32_t)(key >> 32) + 1u));
}

__global__ __launch_bounds__(kRdThreads) void render_resolve_kernel(const unsigned long long* __restrict__ vis, int width, int height,
                                                                     himo_shade sh, unsigned char* __restrict__ rgb) {
    const int p = blockIdx.x * kRdThreads + threadIdx.x;
    if (p >= width * height) return;
    const unsigned long long key = vis[p];
    uint32_t c = sh.background;
    if (key != kRdEmpty) {
        const uint32_t idx = (uint32_t)key;
        c = sh.neutral;
        if ((int64_t)idx < sh.n_attr) {                          // an index no attribute stands behind: neutral
            if (sh.mode == 0) {
                c = sh.rgba[idx];
            } else if (sh.mode == 1) {
                const float s = sh.scalar[idx];
                if (isfinite(s)) {
                    float t = s - sh.lo;
                    t = t * sh.scale;
                    c = sh.lut[(int)fminf(fmaxf(floorf(t), 0.0f), 255.0f)];
                }
            } else {
                const int32_t id = sh.ids[idx];
                if (id >= 0) c = sh.palette[id % sh.palette_n];
            }
        }
    }
    float ch[3] = {(float)(c & 0xFFu), (float)((c >> 8) & 0xFFu), (float)((c >> 16) & 0xFFu)};
    if (key != kRdEmpty && sh.edl_strength > 0.0f) {
        const int x = p % width, y = p / width, e = sh.edl_px;
        const float lc = rd_depth_log(key);
        float sum = 0.0f;
        sum = sum + fmaxf(0.0f, lc - (x - e >= 0 ? rd_depth_log(vis[p - e]) : lc));
        sum = sum + fmaxf(0.0f, lc - (x + e < width ? rd_depth_log(vis[p + e]) : lc));
        sum = sum + fmaxf(0.0f, lc - (y - e >= 0 ? rd_depth_log(vis[p - e * width]) : lc));
        sum = sum + fmaxf(0.0f, lc - (y + e < height ? rd_depth_log(vis[p + e * width]) : lc));
        const float resp = sum / 4.0f;
        const float shade = exp2f(-sh.edl_strength * resp);
#pragma unroll
        for (int k = 0; k < 3; ++k) ch[k] = floorf(ch[k] * shade + 0.5f);
    }
    unsigned char* out = rgb + (int64_t)p * 3;
    out[0] = (unsigned char)ch[0]; out[1] = (unsigned char)ch[1]; out[2] = (unsigned char)ch[2];
}

static bool rd_size_ok(int width, int height) { return width > 0 && height > 0; }

}  // namespace himo

using namespace himo;

extern "C" int himo_render_clear(uint64_t* d_vis, int width, int height, void* stream) {
    if (!rd_size_ok(width, height) || !d_vis || (reinterpret_cast<uintptr_t>(d_vis) & 7u)) return HIMO_ERR_INVALID_ARGUMENT;
    if (width > kRdMaxSide || height > kRdMaxSide) return HIMO_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int cells = width * height;
    {
        ProfScope ps("render_clear_kernel", s);
        hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)((cells + kRdThreads - 1) / kRdThreads)), dim3(kRdThreads), 0, s,
                           reinterpret_cast<unsigned long long*>(d_vis), cells);
    }
    HIMO_LAUNCH_CHECK("render_clear_kernel");
    return HIMO_OK;
}

extern "C" int himo_render_splat(int64_t n, const float* d_pts, int pitch, const float* d_offset, const unsigned char* d_skip,
                                 const himo_camera* cam, int radius, uint32_t index_base, uint64_t* d_vis, void* stream) {
    if (n < 0 || pitch < 3 || radius < 0 || radius > 8 || !cam || !rd_size_ok(cam->width, cam->height)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_vis || (reinterpret_cast<uintptr_t>(d_vis) & 7u) || (n > 0 && !d_pts)) return HIMO_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(d_pts) & 3u) || (reinterpret_cast<uintptr_t>(d_offset) & 3u)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!isfinite(cam->znear) || !isfinite(cam->zfar) || !(cam->zfar > cam->znear) || !isfinite(cam->inv_range) || !(cam->inv_range > 0.f))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (cam->width > kRdMaxSide || cam->height > kRdMaxSide || n > 0x7fffffffLL || (int64_t)index_base + n > 0x100000000LL)
        return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("render_splat_kernel", s);
        hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)((n + kRdThreads - 1) / kRdThreads)), dim3(kRdThreads), 0, s, (int)n, d_pts,
                           pitch, d_offset, d_skip, *cam, radius, index_base, reinterpret_cast<unsigned long long*>(d_vis));
    }
    HIMO_LAUNCH_CHECK("render_splat_kernel");
    return HIMO_OK;
}

extern "C" int himo_render_resolve(const uint64_t* d_vis, int width, int height, const himo_shade* shade, unsigned char* d_rgb,
                                   void* stream) {
    if (!rd_size_ok(width, height) || !d_vis || (reinterpret_cast<uintptr_t>(d_vis) & 7u) || !shade || !d_rgb) return HIMO_ERR_INVALID_ARGUMENT;
    const himo_shade& h = *shade;
    if (h.mode < 0 || h.mode > 2 || h.n_attr < 0) return HIMO_ERR_INVALID_ARGUMENT;
    if (h.mode == 0 && h.n_attr > 0 && !h.rgba) return HIMO_ERR_INVALID_ARGUMENT;
    if (h.mode == 1 && (!h.lut || (h.n_attr > 0 && !h.scalar) || !isfinite(h.lo) || !isfinite(h.scale))) return HIMO_ERR_INVALID_ARGUMENT;
    if (h.mode == 2 && (h.palette_n <= 0 || !h.palette || (h.n_attr > 0 && !h.ids))) return HIMO_ERR_INVALID_ARGUMENT;
    if (!(h.edl_strength >= 0.f) || !isfinite(h.edl_strength) || (h.edl_strength > 0.f && (h.edl_px < 1 || h.edl_px > kRdMaxSide)))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (width > kRdMaxSide || height > kRdMaxSide) return HIMO_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int cells = width * height;
    {
        ProfScope ps("render_resolve_kernel", s);
        hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((cells + kRdThreads - 1) / kRdThreads)), dim3(kRdThreads), 0, s,
                           reinterpret_cast<const unsigned long long*>(d_vis), width, height, h, d_rgb);
    }
    HIMO_LAUNCH_CHECK("render_resolve_kernel");
    return HIMO_OK;
}
