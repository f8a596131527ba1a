// Device helpers of the split-operand arithmetics on the matrix pipe (the story: conv_x6_kernels.hpp): the fragment cell, the
// exact three-part bf16 split ("x6"), the two-part fp16 split ("h3"), their MFMA sequences.  No __global__ function in here.
#pragma once
#include "gemm_f32_mfma.hpp"

namespace tvae {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
union Cell16 {                 // one fragment cell: 8 consecutive-k bf16 (or fp16) of one row (an MFMA operand register quad)
    uint4 u;
    bf16x8 v;
    f16x8 h;
    unsigned w[4];
};

constexpr int X6_STAGE_CELLS_FWD = 3 * 2 * 256;      // [part][octet half][256 rows]
constexpr int X6_STAGE_CELLS_WG = 3 * 2 * 128;       // [part][octet half][128 rows]
constexpr int X6_TAB_BYTES = 64;

static inline int x6_round_up(int v, int q) { return (v + q - 1) / q * q; }
// per-array element count of the LDS image: >= elems + 16 slack, and == 32 (mod 64), i.e. 16 dwords (mod 32): the
// 4-byte reads use 32 banks, and consecutive arrays -- hence also the two parity copies of one part, 3 arrays apart --
// then start 16 banks apart, so the even lanes (copy 0) and odd lanes (copy 1) of a fragment read never collide
static inline int x6_arr_elems(int elems) { return x6_round_up(elems + 16, 64) + 32; }

// exact three-way bf16 split of one fp32 value (RNE residuals); returns the raw bf16 bit patterns
__device__ __forceinline__ void split3(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
    const __bf16 bh = (__bf16)x;
    const float r1 = x - (float)bh;
    const __bf16 bm = (__bf16)r1;
    const float r2 = r1 - (float)bm;
    const __bf16 bl = (__bf16)r2;
    h = __builtin_bit_cast(unsigned short, bh);
    m = __builtin_bit_cast(unsigned short, bm);
    l = __builtin_bit_cast(unsigned short, bl);
}
// the same split for two values at once, results packed (x0 in the low half): v_cvt_pk_bf16_f32 rounds both, the parts
// are widened again with a shift / a mask and the residuals come from one packed subtraction -- 9 VALU instructions
// per pair instead of ~9 per value, bitwise the same parts as split3
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& hw, unsigned& mw, unsigned& lw) {
    const f32x2v x = {x0, x1};
    hw = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2v));
    const f32x2v hf = {__uint_as_float(hw << 16), __uint_as_float(hw & 0xffff0000u)};
    const f32x2v r1 = x - hf;
    mw = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2v));
    const f32x2v mf = {__uint_as_float(mw << 16), __uint_as_float(mw & 0xffff0000u)};
    const f32x2v r2 = r1 - mf;
    lw = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2v));
}
__device__ __forceinline__ void split3x8(const float (&r)[8], Cell16& h, Cell16& m, Cell16& l) {
#pragma unroll
    for (int q = 0; q < 4; ++q) split3_pair(r[2 * q], r[2 * q + 1], h.w[q], m.w[q], l.w[q]);
}

// ------------------------------------------------------------------------------------------
// "h3" arithmetic (round 3): TWO fp16 parts per operand, THREE partial products.
// fp16 carries 11 significant bits (unit roundoff 2^-11), so with round-to-nearest parts  h = fp16(x), l = fp16(x - h)
//   |x - h| <= 2^-11 |x|,   |x - h - l| <= 2^-23 |x|   (as long as l is a normal fp16 number):
// x - h is an fp32 number of at most 13 significant bits, of which l keeps 11 -- two parts represent an fp32 value to ONE
// ulp (exactly, whenever x - h fits 11 bits, which is the common case).  h k + h k' + l k  leaves out  l l' <= 2^-22 |x y|.
// Worst case per product: 2^-23 + 2^-23 + 2^-22 = 2^-21 |x y| -- 8x the rounding of one fp32 FMA, but unbiased and not
// accumulating through the sum the way an FMA chain's own roundings do: products of fp16 numbers are exact in the fp32
// accumulator (22 bits).  What carries the accuracy claim is therefore the MEASUREMENT, not this bound: against fp64 the
// result is at least as accurate as the fp32 matrix pipe and as the six-product bf16 split for every distribution and
// reduction length probed (profiles/experiments/f16_split_probe.hip: 2.6e-7 vs 4.1e-7 (fp32 MFMA) vs 3.5e-7 (x6) at
// K = 512), with HALF the matrix instructions of x6.
// The price is fp16's 5-bit exponent: an operand is multiplied by a power of two (exact) that brings the largest
// magnitude of its scale group -- or an upper bound of it -- into [2^14, 2^15), and the accumulators by the inverse powers
// in the epilogue.  An element 2^j below the maximum of its group keeps min(23, 39 - j) significant bits (beyond j = 16
// the low part enters fp16's subnormal range, absolute error 2^-25 of the scaled value): 2^-16 -> exact, 2^-24 -> 3e-5,
// 2^-28 -> 5e-4 relative to ITSELF.  Round 3 used ONE group per operand tensor, which is fine normwise but lets a whole
// row of small values (a dead unit, a dim image) come out with few correct bits.  Round 4: the scale group is a ROW of the
// operand in the sense of the product (H3Scale, dense_x6_kernels.hpp) wherever its producer can supply row maxima -- a
// row / column of the OUTPUT then has the full two-part precision relative to its own magnitude, and what remains under
// one scale is the reduction index, where an element far below its row's maximum is negligible in the sum it enters
// (error <= 2^-39 of max_row |a| max_col |b| per term).  The remaining per-tensor scales and why they are safe are listed
// in DESIGN.md section 4 ("validity domain of h3"); tests/test_hip_primitives.py::test_h3_row_dynamic_range holds rows
// scaled by 2^-16 .. 2^-32 to 1e-5 per row against fp64.
// ------------------------------------------------------------------------------------------
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
// the power of two s with 2^14 <= s * amax < 2^15 (amax = 0, or absurdly small / large: clamped, s stays a normal number
// whose inverse is one too)
__device__ __forceinline__ float h3_scale(float amax) {
    int e = (int)((__float_as_uint(amax) >> 23) & 0xffu);        // amax in [2^(e-127), 2^(e-126))
    if (e == 0) e = 127;                                         // zero (or denormal) maximum: scale 2^14
    int se = 268 - e;                                            // biased exponent of 2^(14 - (e - 127))
    se = se < 2 ? 2 : (se > 252 ? 252 : se);
    return __uint_as_float((unsigned)se << 23);
}
__device__ __forceinline__ float h3_inv(float s) {               // 1 / s for a power of two produced by h3_scale
    return __uint_as_float((254u - (__float_as_uint(s) >> 23)) << 23);
}
// both parts of two (already scaled) values at once, packed (x0 in the low half)
__device__ __forceinline__ void split2h_pair(float x0, float x1, unsigned& hw, unsigned& lw) {
    const f32x2v x = {x0, x1};
    const f16x2v h = __builtin_convertvector(x, f16x2v);
    hw = __builtin_bit_cast(unsigned, h);
    const f32x2v hf = __builtin_convertvector(h, f32x2v);
    const f32x2v r = x - hf;
    lw = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2v));
}
__device__ __forceinline__ void split2hx8(const float (&r)[8], Cell16& h, Cell16& l) {
#pragma unroll
    for (int q = 0; q < 4; ++q) split2h_pair(r[2 * q], r[2 * q + 1], h.w[q], l.w[q]);
}
// three partial products; the small ones first is not needed (see mfma6)
__device__ __forceinline__ void mfma3h(f32x16& acc, const Cell16 (&a)[3], const Cell16 (&b)[3]) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0].h, b[0].h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0].h, b[1].h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1].h, b[0].h, acc, 0, 0, 0);
}
// max |x| into a device word by atomic max on the bit pattern (non-negative floats order like unsigned integers); NaN
// / Inf propagate as a huge maximum -> scale clamped, the result is then non-finite as it would be in any arithmetic
__device__ __forceinline__ void h3_atomic_amax(float* slot, float v) {
    const unsigned b = __float_as_uint(fabsf(v));
    // most callers arrive with less than what is already there: a plain read spares the L2 their atomic
    if (b > __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(slot))) atomicMax(reinterpret_cast<unsigned*>(slot), b);
}
__device__ __forceinline__ float h3_wave_max(float v) {          // in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Round 4 (h3 scales per row): the transforms along w leave one maximum per filter row / channel.  A wave's running
// maximum is flushed into the slot of a row when the wave moves on to another row (and at its end): wave reduction, then ONE
// atomic without return from lane 0.  (A first version flushed after every tile: 270 000 atomics on the 128 words = four
// cache lines of the channel maxima serialised in the memory system and DOUBLED the output transform, 0.83 -> 1.51 ms; the
// ring kernels now walk contiguous tile ranges, so a wave sees at most a handful of rows.)  In the ring kernels the atomic
// is NOT part of the hand-counted waits: a wait that does not know about it merely asks for one more of the oldest stores.
__device__ __forceinline__ void h3_tile_flush(float& mx, float* slot, int lane) {
    const float m = h3_wave_max(mx);
    if (lane == 0) __hip_atomic_fetch_max(reinterpret_cast<unsigned*>(slot), __float_as_uint(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mx = 0.f;
}
// the same where the kernel's loads are the compiler's to count (generic / register-staged transforms, whose tiles go round
// robin): read first, most tiles bring nothing new
__device__ __forceinline__ void h3_tile_flush_rd(float& mx, float* slot, int lane) {
    const float m = h3_wave_max(mx);
    if (lane == 0) h3_atomic_amax(slot, m);
    mx = 0.f;
}

// block-wide maximum, then ONE atomic per workgroup (per-wave atomics on a single word serialise at the L2: 12 000 of
// them made a 5 us reduction take 140).  Every thread of the workgroup must call it.
__device__ __forceinline__ void h3_block_amax(float v, float* slot) {
    __shared__ float red_[16];
    v = h3_wave_max(v);
    __syncthreads();                                             // red_ may still be read by the previous call
    if ((threadIdx.x & 63) == 0) red_[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = red_[0];
        for (int i = 1; i < (int)((blockDim.x + 63) >> 6); ++i) m = fmaxf(m, red_[i]);
        h3_atomic_amax(slot, m);
    }
}

// six partial products, in the order the A parts arrive from LDS (h, m, l): the first MFMA of a fragment then waits
// for ONE read, not three (the running sum already dwarfs every term, so the order is irrelevant for accuracy)
__device__ __forceinline__ void mfma6(f32x16& acc, const Cell16 (&a)[3], const Cell16 (&b)[3]) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0].v, b[0].v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0].v, b[1].v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0].v, b[2].v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1].v, b[0].v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1].v, b[1].v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2].v, b[0].v, acc, 0, 0, 0);
}

}  // namespace tvae
