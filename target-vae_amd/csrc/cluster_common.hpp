// What the kernel families of libtvae_cluster.so share: the launch check, the host-side argument tests that do not belong
// to one family (finite, the mask, the byte spans of the pointer arguments and their overlap rules; the shape range of the
// pose searches is refine_device.hpp's), the shape limits, the DFT twiddle table and the fragment conventions of the fp32 MFMA.  Host and device code, and NO __global__ function:
// a non-template kernel is emitted by every unit that sees its definition (abi_common.hpp), so a header that any unit of the
// library may include -- this one -- must not define one.  That is the difference from align_kernels.hpp and the other
// *_kernels.hpp, each of which exactly one unit may see.  It does not include abi_common.hpp either: that header carries the
// training ABI and gemm_f32_mfma.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tvae_cluster.h"

#define TVAE_CLUSTER_CHECK_LAUNCH()              \
    do {                                         \
        hipError_t e__ = hipGetLastError();      \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

namespace tvae_cluster {

// ---- host ------------------------------------------------------------------------------------------------------------------
constexpr long GRID_MAX = 0x7fffffffL;   // workgroups along x of one launch

static inline hipStream_t S(tvae_stream_t s) { return (hipStream_t)s; }
static inline bool aligned8(const void* p) { return (reinterpret_cast<size_t>(p) & 7) == 0; }
static inline bool finite(float x) { return x - x == 0.f; }            // false for NaN and +-inf
static inline bool mask_ok(float radius, float edge) { return finite(radius) && finite(edge) && edge >= 0.f; }

// A pointer argument and the bytes the call reads or writes behind it.  A null pointer -- an optional argument that was left
// away; the required ones are tested before -- overlaps nothing.
struct Span {
    const void* p;
    size_t bytes;
};
static inline bool overlap(Span a, Span b) {
    const size_t x = reinterpret_cast<size_t>(a.p), y = reinterpret_cast<size_t>(b.p);
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}
// no output shares a byte with an input
template <int NO, int NI>
static inline bool outputs_off_inputs(const Span (&out)[NO], const Span (&in)[NI]) {
    for (const Span& o : out)
        for (const Span& i : in)
            if (overlap(o, i)) return false;
    return true;
}
// ... and no two outputs share one either
template <int NO, int NI>
static inline bool outputs_clear(const Span (&out)[NO], const Span (&in)[NI]) {
    for (int a = 0; a < NO; ++a)
        for (int b = a + 1; b < NO; ++b)
            if (overlap(out[a], out[b])) return false;
    return outputs_off_inputs(out, in);
}
// (allow_big_lds of abi_common.hpp)
template <class KernelT>
static hipError_t allow_big_lds(KernelT kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

// ---- limits: one set for every family; a family header names a limit of its own only where it means something else -----------
constexpr int SIDE_MAX = 1024;           // n: side of an image or plane
constexpr int PLANES_MAX = 1 << 24;      // images or planes of a stack
constexpr int CLASSES_MAX = 65535;       // classes

// ---- bilinear sampling with a zero border, and the soft circular mask --------------------------------------------------------
// The sample of img[n][n] at the position (row, col) in pixels: the taps floor and floor + 1 per axis, a tap outside
// [0, n - 1] is 0, and a position that is not inside (-1, n) on both axes gives exactly 0 -- the range is tested BEFORE the
// float -> int conversion and NaN fails it.  `on` = false gives 0 as well; nothing but in-bounds words is ever read.
__device__ __forceinline__ bool inside_frame(float col, float row, int n) {
    const float fn = (float)n;
    // NaN fails every comparison: false for NaN, +-inf and anything that would not convert to an int
    return (col > -1.f) && (col < fn) && (row > -1.f) && (row < fn);
}

__device__ __forceinline__ float bilinear_zero_border(const float* __restrict__ img, int n, float col, float row, bool on) {
    const bool in = on && inside_frame(col, row, n);
    const float colc = in ? col : 0.f, rowc = in ? row : 0.f;
    const float fc = floorf(colc), fr = floorf(rowc);
    const int c0 = (int)fc, r0 = (int)fr;                     // in [-1, n - 1]
    const float wc = colc - fc, wr = rowc - fr;
    const bool c0in = c0 >= 0, c1in = c0 + 1 <= n - 1, r0in = r0 >= 0, r1in = r0 + 1 <= n - 1;
    const int ca = c0in ? c0 : 0, cb = c1in ? c0 + 1 : n - 1;
    const int ra = r0in ? r0 : 0, rb = r1in ? r0 + 1 : n - 1;
    const float v00 = img[ra * n + ca], v01 = img[ra * n + cb], v10 = img[rb * n + ca], v11 = img[rb * n + cb];
    const float a00 = (in && r0in && c0in) ? v00 : 0.f, a01 = (in && r0in && c1in) ? v01 : 0.f;
    const float a10 = (in && r1in && c0in) ? v10 : 0.f, a11 = (in && r1in && c1in) ? v11 : 0.f;
    const float top = fmaf(wc, a01 - a00, a00);
    const float bot = fmaf(wc, a11 - a10, a10);
    return fmaf(wr, bot - top, top);
}

// The pose of an image in the convention of align_kernels.hpp, and the bilinear sample of img[n][n] at the canonical pixel
// (i, j) under it; `on` = false gives 0 without reading anything else than in-bounds words.
struct AlignPose {
    float c, s, tx, ty;                  // cos, sin, t * dx0, t * dx1
};

__device__ __forceinline__ float align_sample(const float* __restrict__ img, int n, int i, int j, float step, float half,
                                              const AlignPose p, bool on) {
    const float u0 = fmaf((float)j, step, -1.f);
    const float u1 = fmaf(-(float)i, step, 1.f);
    const float x0 = fmaf(u0, p.c, fmaf(u1, p.s, p.tx));
    const float x1 = fmaf(-u0, p.s, fmaf(u1, p.c, p.ty));
    const float col = (x0 + 1.f) * half;
    const float row = (1.f - x1) * half;
    return bilinear_zero_border(img, n, col, row, on);
}

// ---- the chunks of a class and their workspace slots --------------------------------------------------------------------------
// THE statement of the slot numbering of the class averages, the eigenimages and the weighted averages.  `clean` is a monotone
// seg[K + 1]; class k = the positions [s_k, e_k) is cut into chunks of `chunk` positions counted from s_k, and chunk c owns the
// slot floor(s_k / chunk) + k + c: slots of different classes never collide, and there are at most total / chunk + K of them.
// chunk_of_slot finds the chunk that owns `slot`: its class, its first position and its length.  false for a slot that no
// chunk owns (nobody reads such a slot either); the answer depends on `slot` and `clean` alone, so it is uniform over a
// workgroup whose slot comes from blockIdx.  `chunk` is a constant at every call site: the divisions are by a constant.
struct ChunkSpan {
    int k, first, members;
};

__device__ __forceinline__ bool chunk_of_slot(const int* __restrict__ clean, int K, int slot, int chunk, ChunkSpan& out) {
    // the class whose slots contain `slot`: the largest k with clean[k] / chunk + k <= slot (strictly increasing in k)
    int lo = 0, hi = K - 1;
    if (clean[0] / chunk > slot) return false;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (clean[mid] / chunk + mid <= slot) lo = mid; else hi = mid - 1;
    }
    const int sk = clean[lo], ek = clean[lo + 1];
    const int first = sk + (slot - (sk / chunk + lo)) * chunk;
    if (first >= ek) return false;
    out.k = lo;
    out.first = first;
    out.members = min(chunk, ek - first);
    return true;
}

// The mask at d pixels from the centre for radius > 0: 1 within `radius`, a raised cosine over `edge`, 0 beyond.
__device__ __forceinline__ float soft_mask(double d, float radius, float edge) {
    const double r = (double)radius, e = (double)edge;
    if (d <= r) return 1.f;
    if (d >= r + e) return 0.f;                               // (edge = 0: a hard edge, never the division below)
    return (float)(0.5 * (1.0 + cospi((d - r) / e)));
}

// m(i, j): 1 within `radius` of the centre ((n - 1) / 2, (n - 1) / 2), a raised cosine over `edge`, 0 beyond; radius <= 0: no
// mask.  fp64: what the mask adds to the error of a coefficient is far below the sums' own rounding.
__device__ __forceinline__ float frc_mask(int i, int j, int n, float radius, float edge) {
    if (!(radius > 0.f)) return 1.f;
    const double c = 0.5 * (double)(n - 1);
    const double di = (double)i - c, dj = (double)j - c;
    return soft_mask(sqrt(di * di + dj * dj), radius, edge);
}

// ---- rings of a spectrum: r - 1/2 <= sqrt(ks^2 + kx^2) < r + 1/2, decided in integers -----------------------------------------
// the least kx >= 0 with 4 kx^2 >= t (t below 2^23: exact in fp32, and the two loops make the estimate exact)
__device__ __forceinline__ int frc_first_kx(int t) {
    if (t <= 0) return 0;
    int kx = (int)ceilf(0.5f * sqrtf((float)t));
    while (kx > 0 && 4 * (kx - 1) * (kx - 1) >= t) --kx;
    while (4 * kx * kx < t) ++kx;
    return kx;
}

// the ring of s2 = ks^2 + kx^2 (at most 2 * 512^2: exact in fp32): the r with (2r - 1)^2 <= 4 s2 < (2r + 1)^2, 0 for s2 = 0
__host__ __device__ static inline int ring_of(int s2) {
    int r = (int)(sqrtf((float)s2) + 0.5f);
    while ((2 * r + 1) * (2 * r + 1) <= 4 * s2) ++r;
    while (r > 0 && (2 * r - 1) * (2 * r - 1) > 4 * s2) --r;
    return r;
}

// ---- direct DFT --------------------------------------------------------------------------------------------------------------
// kx = 0 .. n / 2 of a half spectrum; also the number of rings
__host__ __device__ static inline int half_side(int n) { return n / 2 + 1; }

// The n twiddles (cos, sin)(2 pi t / n) of a workgroup: sincospi in fp64 on the exact argument 2 t / n, rounded to fp32 once
// (half an ulp; exact 0 and +-1 on the axes).  `stride` = the threads of the workgroup, a constant or blockDim.x.
__device__ __forceinline__ void dft_twiddles(float2* tw, int n, unsigned stride) {
    for (int t = threadIdx.x; t < n; t += stride) {
        double s, c;
        sincospi((double)(2 * t) / (double)n, &s, &c);
        tw[t] = make_float2((float)c, (float)s);
    }
}

// t = (a k) mod n from one k to the next, in integers: t and step in [0, n), no argument is ever reduced in floating point
__device__ __forceinline__ void tw_advance(int& t, int step, int n) {
    t += step;
    t -= t >= n ? n : 0;
}

// ---- v_mfma_f32_32x32x2_f32: an exact fp32 FMA chain per output, ascending k -----------------------------------------------------
// Lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].  D is sixteen registers per lane: column
// j = l & 31, row i = mfma_row(reg, l >> 5) = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) (gemm_f32_mfma.hpp).
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// row of accumulator register r within a tile whose first row is row0 (row0 is added FIRST, as the kernels always wrote the
// sum: another order of the integer additions is another instruction schedule)
__device__ __forceinline__ int mfma_row(int r, int khalf, int row0 = 0) {
    return row0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
}

}  // namespace tvae_cluster
