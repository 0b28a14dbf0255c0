// Split-bf16 ("bf16x6") GEMM core for float32 operands on gfx950 (MI355X).
//
//   C(m, n) = sum_k A(m, k) * B(k, n)        (float32 in, float32 accumulate)
//
// The fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 MFMA rate and gfx950 has no xf32.
// This core splits every fp32 operand, with round-to-nearest, into three bf16 planes
//     a = h + m + l + r,   h = bf16(a),  m = bf16(a - h),  l = bf16(a - h - m)
// (|m| <= 2^-9 |a|, |l| <= 2^-18 |a|, |r| <= 2^-27 |a|; bf16 has the exponent range of fp32, so no
// scaling) and accumulates the six products  lh + hl + mm + mh + hm + hh  per 16-deep K block with
// v_mfma_f32_32x32x16_bf16 into the fp32 accumulator.  A bf16 x bf16 product is exact in fp32; the
// dropped terms (ml, lm, ll and the r parts) sum to about 2^-26 sum|a||b|, under the 2^-24 unit roundoff
// of the fp32 accumulation itself, so the error has the norm-wise form and size of the fp32 core's.
// Except for tiny operands: below 2^-126 a bf16 is subnormal, on a 2^-133 grid, so once |a| < ~2^-108 (l) or
// ~2^-117 (m) the planes hold a only to ~2^-134 absolutely.  The MFMA keeps bf16 subnormal inputs, and the bound
// gains an absolute floor:  |C - C64| <= (fp32 size) sum_k |a||b| + 2^-133 (sum_k |a_ik| + sum_k |b_kj|).
// It is the plain relative bound down to 2^-113; at 2^-120 the relative error reaches ~6e-6, at 2^-126 ~5e-4
// (K = 256, random signs; DESIGN section 4, tests/test_gpu_bf16x6_range.py).
// Six bf16 MFMAs (6 x 32 cycles) do the work of sixteen fp32 ones (16 x 64 cycles).
//
// Same problem description (GemmProblem), tile map (xcd_remap, mt_fast, two-segment B, split-K ranges)
// and epilogue functors as gemm_mfma_f32.hpp; only the aligned fast path (whole tiles, 16-deep K blocks,
// 16-byte aligned K-major operands) exists here -- x6_eligible() says when, and the callers keep the fp32
// core otherwise.
//
// Staging: fp32 panels go global -> registers, are split into the three planes in registers
// (v_cvt_pk_bf16_f32 and an fp32 residual) and written to another LDS buffer; one barrier per K block.
// Global -> LDS DMA cannot transform data.  The split runs inside the MFMA stream: during block kb a wave
// issues the first 2 TN products of each 32-row A block, then splits and stores one panel of a later block
// (A panel in the first A block, B panel in the second) and issues that panel's next loads, then the other
// 4 TN products, so the waves of a SIMD do not all split with the matrix pipe idle (the 62 % pipe-busy body
// of round 6).  The register ring stays one block deep: the split frees ra / rb before the loads refill them.
//   128 x 128 tile: two LDS buffers (three would cost one of its three workgroups per CU).  Block kb + 1 is
//     staged during block kb, the loads run two blocks ahead, and the barrier sits between the blocks: every
//     wave leaves it needing its first fragments at once.
//   256 x 256 tile: a ring of three buffers (3 x 48 KiB; one workgroup per CU either way).  Block kb + 2 is
//     staged during block kb, the loads run three blocks ahead, and the barrier sits inside the block, after a
//     wave's last fragment read of the block and its second group's first product.  The waves cross the block
//     boundary staggered by the matrix pipe instead of aligned by a barrier, and the fragment registers are
//     refilled one plane at a time as the fixed term order lets them die (group 0: the second group's A
//     fragments; group 1, behind the barrier: the next block's fragments from the next buffer), so fragment
//     reads are spread through the MFMA stream and a block starts with only its h planes on the way (the
//     conditions are at the K loop).
//   KMAJOR panel (reduction index contiguous): one 16-byte load = 4 k of one row.
//     LDS image of one plane: [rows][16 k] bf16, 32 bytes per row, two 16-byte chunks (k 0..7, 8..15);
//     chunk q of row r sits at chunk q ^ ((r >> 3) & 1).  A lane (l31, h) of the 32x32x16 MFMA reads
//     chunk h of its row with one ds_read_b128; the four ds_read_b128 lane groups of MI355X_MICROARCH
//     then each hit 16 distinct 16-byte slots (conflict free).
//   XMAJOR panel (row index contiguous: x^T, [Y | x] of the reduction over samples): one 16-byte load =
//     4 consecutive rows at one k (a wave reads 1 KiB of one k row).  LDS image of one plane: [16 k][rows]
//     bf16 in 8-byte granules of 4 rows; granule g of k row k sits at g ^ (8 (k & 3)).  The split writes
//     each plane's granule with one ds_write_b64; the fragment is read back transposed with two
//     ds_read_b64_tr_b16 (k 8h..8h+3 and 8h+4..8h+7).  A 32-lane half of one such read takes 4 k rows
//     x 8 granules; the XOR puts them on 32 distinct bank pairs (conflict free).
//
// Denominator tail (256 x 256 NT tile, epilogue functors with kDenTail: the NMF x update): after the K loop the
// workgroup forms its own tile of x.G on the fp32 MFMA, through the freed LDS ring and in the exact order of the
// stand-alone fp32 product, and applies the MU quotient to the accumulators; x.G is never stored.  Described at
// x6_den_tail() below.  The K loop, its ring and its barriers are the same code for every functor.
#pragma once
#include "gemm_mfma_f32.hpp"
#include <type_traits>

namespace dcp {

// Diagnostic build only (-DDCP_X6_STAMPS on the translation unit that launches the kernel; off by default, so no
// stamp runs in the shipped kernel): the 256 x 256 K loop reads the shader clock at four places per K block, keeps
// the sums in scalar registers, and lane 0 of every wave of workgroup 0 stores them once after the loop into
// x6_stamp_buf[wave][8] = { cycles from the previous block's last MFMA (the first block: from the prologue's
// fragment reads) to the operands of the block's first MFMA, cycles from the last MFMA of group 0 to the barrier's
// exit (group 1's first product lies in between), cycles between the first and the last stamped block start,
// stamped blocks, cost of one stamp }.  Each stamp drains lgkmcnt (s_memtime returns through it), so the build is
// slower than the real one and only its shares mean anything.  tools/bf16x6_stamps.py reads the buffer.
#ifdef DCP_X6_STAMPS
static __device__ unsigned long long x6_stamp_buf[16 * 8];
#define X6_STAMP(t)                                                                         \
    do {                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                  \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");        \
        __builtin_amdgcn_sched_barrier(0);                                                  \
    } while (0)
#endif

typedef __bf16 x6_bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 x6_bf16x8 __attribute__((ext_vector_type(8)));

// 64-row wave tiles of 32x32 accumulator blocks, 16-deep K blocks
template <int BM_, int BN_, int WM_, int WN_, int MINW_, int STAGES_>
struct X6Cfg {
    static constexpr int BM = BM_, BN = BN_, BK = 16, WM = WM_, WN = WN_, MINW = MINW_;
    static constexpr int NWAVES = (BM_ / WM_) * (BN_ / WN_);
    static constexpr int NTHREADS = 64 * NWAVES;
    static constexpr int STAGES = STAGES_;   // LDS buffers of planes: 2 (barrier between K blocks) or a ring of 3
};
typedef X6Cfg<256, 256, 64, 64, 1, 3> X6Huge;    // 16 waves, 3 x 48 KiB of planes, one workgroup per CU
typedef X6Cfg<128, 128, 64, 64, 2, 2> X6Large;   // 4 waves, 2 x 24 KiB of planes (a third would cost a workgroup per CU)

template <int ROWS>
struct X6Panel {
    static constexpr int PLANE_BYTES = ROWS * 32;
    static constexpr int BYTES = 3 * PLANE_BYTES;
};

// byte offset of chunk q (8 k) of row r inside one plane
__device__ __forceinline__ int x6_chunk(int r, int q) { return r * 32 + ((q ^ ((r >> 3) & 1)) << 4); }

// the three planes of 4 fp32 values
__device__ __forceinline__ void x6_split(f32x4 a, x6_bf16x4& h, x6_bf16x4& m, x6_bf16x4& l) {
    h = __builtin_convertvector(a, x6_bf16x4);
    const f32x4 r1 = a - __builtin_convertvector(h, f32x4);      // exact: a - round(a)
    m = __builtin_convertvector(r1, x6_bf16x4);
    const f32x4 r2 = r1 - __builtin_convertvector(m, f32x4);     // exact
    l = __builtin_convertvector(r2, x6_bf16x4);
}

// G = groups of 4 values per thread per K block (KMAJOR: 4 k of one row; XMAJOR: 4 rows at one k)
// SBASE (the 256 x 256 ring, which has no registers to spare): scalar base + 32-bit thread offset, see below.
template <int LAY, int ROWS, int NT, bool SBASE, int G>
__device__ __forceinline__ void x6_gload(f32x4 (&r)[G], const float* __restrict__ p, long ld, int row0, int k0,
                                         int tid) {
    static_assert(G * NT * 4 == ROWS * 16, "panel must be a whole number of 4-value groups per thread");
    if constexpr (!SBASE) {
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int idx = tid + i * NT;
            if (LAY == KMAJOR) {
                const int row = idx >> 2, kq = idx & 3;
                r[i] = *reinterpret_cast<const f32x4*>(p + (long)(row0 + row) * ld + (k0 + 4 * kq));
            } else {
                const int g = idx % (ROWS / 4), k = idx / (ROWS / 4);
                r[i] = *reinterpret_cast<const f32x4*>(p + (long)(k0 + k) * ld + (row0 + 4 * g));
            }
        }
        return;
    }
    // The block's part of the address is uniform; the thread's part fits 32 bits (x6_eligible) and is the same
    // for every K block: one VGPR per load, where a flat address costs a 64-bit pointer and a 64-bit k offset per
    // panel.  The empty asm keeps the uniform part in SGPRs: without it hipcc adds the two in the other order and
    // carries the sum in VGPRs through the loop.
    // These pins (here, on `off` below and in ring_off of the kernel) are what holds the 256 x 256 instantiations at
    // 127-128 VGPRs, 0 AGPRs, no scratch and no spills (147 456 B LDS, 4 waves per SIMD) with global_load ... v, s[]
    // loads and no flat_load, read from the ISA of ROCm 7's hipcc: check those figures again after a toolchain
    // update (-Rpass-analysis=kernel-resource-usage, or the metadata at the end of --save-temps' .s).
    // (global address space spelled out: behind the asm hipcc no longer infers it and would issue flat loads)
    typedef const __attribute__((address_space(1))) char* gchar_ptr;
    typedef const __attribute__((address_space(1))) f32x4* gf32x4_ptr;
    gchar_ptr base = (gchar_ptr)(p + (LAY == KMAJOR ? (long)row0 * ld + k0 : (long)k0 * ld + row0));
    asm("" : "+s"(base));
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int idx = tid + i * NT;
        unsigned off;
        if (LAY == KMAJOR) off = (unsigned)(idx >> 2) * (unsigned)ld + 4u * (idx & 3);
        else off = (unsigned)(idx / (ROWS / 4)) * (unsigned)ld + 4u * (idx % (ROWS / 4));
        off *= 4u;
        asm("" : "+v"(off));   // (the widening stays beside the load, where hipcc folds it into the instruction)
        r[i] = *(gf32x4_ptr)(base + off);
    }
}

// XMAJOR image: byte offset of granule g (rows 4g .. 4g+3) of k row k inside one plane
template <int ROWS>
__device__ __forceinline__ int x6_granule(int k, int g) {
    static_assert(ROWS >= 128, "the XOR swizzle needs 32 granules per k row");
    return k * (ROWS * 2) + ((g ^ ((k & 3) << 3)) << 3);
}

template <int LAY, int ROWS, int NT, int G>
__device__ __forceinline__ void x6_lds_store(char* s, const f32x4 (&r)[G], int tid) {
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int idx = tid + i * NT;
        int off;
        if (LAY == KMAJOR) {
            const int row = idx >> 2, kq = idx & 3;
            off = x6_chunk(row, kq >> 1) + ((kq & 1) << 3);
        } else {
            off = x6_granule<ROWS>(idx / (ROWS / 4), idx % (ROWS / 4));
        }
        x6_bf16x4 h, m, l;
        x6_split(r[i], h, m, l);
        *reinterpret_cast<x6_bf16x4*>(s + off) = h;
        *reinterpret_cast<x6_bf16x4*>(s + X6Panel<ROWS>::PLANE_BYTES + off) = m;
        *reinterpret_cast<x6_bf16x4*>(s + 2 * X6Panel<ROWS>::PLANE_BYTES + off) = l;
    }
}

// Byte offset, inside one plane, of this lane's part of the 32x32x16 operand fragment of rows r0 .. r0+31
// (lane (l31, h) holds row l31, k 8h .. 8h+7).  KMAJOR: the ds_read_b128 address.  XMAJOR: the address of
// the first ds_read_b64_tr_b16 -- lane 4q+p of each 16-lane group names k row 8h + q, granule of rows
// r0 + 16 ((lane >> 4) & 1) + 4p .. +3, and receives its row's four k; the second read is 4 k rows on.
template <int LAY, int ROWS>
__device__ __forceinline__ int x6_frag_off(int r0, int lane) {
    const int l31 = lane & 31, h = lane >> 5;
    if (LAY == KMAJOR) return x6_chunk(r0 + l31, h);
    const int q = (lane >> 2) & 3, pq = lane & 3, gh = (lane >> 4) & 1;
    return x6_granule<ROWS>(8 * h + q, (r0 >> 2) + 4 * gh + pq);
}

// The fragment 32 rows on, from the byte offset of a fragment whose r0 is a multiple of 64 (any plane and buffer
// base included: they are multiples of 128).  KMAJOR: 32 rows of 32 bytes, and (r >> 3) & 1 is the same.  XMAJOR: 8
// granules on; bit 3 of the granule index is clear before the swizzle, so the step is a flip of that bit: 64 bytes.
// One offset per panel then serves both 32-row blocks, where two would each hold a register through the K loop.
template <int LAY>
__device__ __forceinline__ int x6_frag_next32(int off) { return LAY == KMAJOR ? off + 32 * 32 : off ^ 64; }

template <int LAY, int ROWS>
__device__ __forceinline__ x6_bf16x8 x6_frag(const char* plane, int off) {
    if (LAY == KMAJOR) return *reinterpret_cast<const x6_bf16x8*>(plane + off);
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    // (every lane takes part: the gather crosses lanes, so EXEC must be all ones here)
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane + off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane + off + 4 * ROWS * 2));
    return __builtin_bit_cast(x6_bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- fused denominator tail (256 x 256 NT tile, functors with `static constexpr bool kDenTail = true`) ----
// The NMF x update needs  x_new = x o max(Y.D^T, 0) / max(x.G, eps).  With such a functor the workgroup, after its
// bf16x6 K loop has left num = Y.D^T in the accumulators, forms its own 256 x 256 tile of den = x.G on the fp32
// MFMA and applies the quotient; den never reaches memory.  The functor carries
//     const float* cur; long ld_cur      x (left operand of x.G and the quotient's multiplicand)
//     const float* gram; long ld_gram    G, [depth, >= n0 + 256] row-major
//     int depth                          reduction depth of x.G (the atom count), a multiple of 16
//     void quot4(int row, int col0, f32x4 num, f32x4 den) const
// Bits: every element of den starts at 0 and takes v_mfma_f32_32x32x2_f32 over K blocks of 16 in ascending
// order, inside a block c = 0, 1 then s = 0 .. 3, the lane halves h supplying k = 8c + 4h + s: the sequence of
// gemm_mfma_kernel<TileCfg<256, 256, 16, 64, 64, 1>, KMAJOR, XMAJOR> (its PIPE == 0 loop, panel_frag), so den is
// bitwise the stand-alone product's.  Nothing assumes G symmetric.
// Registers: num holds 64 of the wave's 128; den is formed in two passes of 32 x 64 per wave (32 registers), pass i
// over the wave's i-th 32-row block, i.e. 128 of the tile's 256 rows per pass, and the quotient of those rows runs
// at the end of their pass.
// LDS: the ring of the K loop is free after one barrier.  A stage is one 16-deep K block of one pass: the x panel
// [128 rows][16 k] (8 KiB, 16-byte chunks XOR-swizzled as the fp32 core's KMAJOR image) and the G panel
// [16 k][256 columns] (16 KiB), in a ring of three 24 KiB buffers with the K loop's barrier argument: during stage
// t a wave issues the 8 MFMAs of c = 0, stores stage t + 2 (in registers since stage t - 1), reads its c = 1
// fragments, passes the barrier, issues the loads of stage t + 3 and then the 8 MFMAs of c = 1.  The stage index
// runs through both passes, so pass 1's first panels are loaded and stored before pass 0's quotient and x_new
// drains under pass 1's MFMAs.  Loads past the last stage re-read it into a buffer nobody reads (no branches).
// Each x element is staged once, G once per pass (it stays in L2).
template <class E, class = void>
struct epi_den_tail { static constexpr bool value = false; };
template <class E>
struct epi_den_tail<E, decltype((void)E::kDenTail)> { static constexpr bool value = E::kDenTail; };

typedef float x6_f32x2 __attribute__((ext_vector_type(2)));

// float offset of 16-byte chunk q (4 k) of row r in the tail's x panel
__device__ __forceinline__ int x6_den_xoff(int r, int q) { return r * 16 + ((q ^ ((r >> 2) & 3)) << 2); }

template <class Epi>
__device__ __forceinline__ void x6_den_tail(f32x16 (&num)[2][2], const Epi& epi, char* smem, int m0, int n0, int tid) {
    constexpr int XS = 128 * 16 * 4;     // x panel of one stage, bytes
    constexpr int GS = 16 * 256 * 4;     // G panel
    constexpr int DBUF = XS + GS;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int l31 = lane & 31, h = lane >> 5;
    const int nkd = epi.depth >> 4;      // K blocks per pass; stages 0 .. 2 nkd - 1

    // staging: a thread moves 8 bytes of the x panel (row pr = 32 wm' + r: tile row 64 wm' + 32 pass + r) and 16
    // bytes of the G panel (a wave moves one k row of it)
    const int pr = tid >> 3, k2 = tid & 7;
    const float* xsrc = epi.cur + (long)(m0 + (pr >> 5) * 64 + (pr & 31)) * epi.ld_cur + 2 * k2;
    const int xdst = (x6_den_xoff(pr, k2 >> 1) + 2 * (k2 & 1)) * 4;
    const int gk = tid >> 6, gc = tid & 63;
    const float* gsrc = epi.gram + (long)gk * epi.ld_gram + (n0 + 4 * gc);
    const int gdst = XS + (gk * 256 + 4 * gc) * 4;
    int lp = 0, lk = 0;                  // pass and K block of the next stage to load (stops at the last one)
    auto gload = [&](x6_f32x2& rx, f32x4& rg) {
        rx = *reinterpret_cast<const x6_f32x2*>(xsrc + (long)(32 * lp) * epi.ld_cur + 16 * lk);
        rg = *reinterpret_cast<const f32x4*>(gsrc + (long)(16 * lk) * epi.ld_gram);
        if (lk + 1 < nkd) {
            ++lk;
        } else if (lp == 0) {
            lp = 1;
            lk = 0;
        }
    };
    auto lstore = [&](int buf, const x6_f32x2& rx, const f32x4& rg) {
        *reinterpret_cast<x6_f32x2*>(smem + buf + xdst) = rx;
        *reinterpret_cast<f32x4*>(smem + buf + gdst) = rg;
    };

    x6_f32x2 rx;
    f32x4 rg;
    int b0 = 0, b1 = DBUF, b2 = 2 * DBUF;   // byte offsets of the buffers of stages t, t + 1, t + 2
    {
        x6_f32x2 rx0, rx1;
        f32x4 rg0, rg1;
        gload(rx0, rg0);
        gload(rx1, rg1);
        gload(rx, rg);
        __syncthreads();   // every wave has left the K loop: the ring is free
        lstore(b0, rx0, rg0);
        lstore(b1, rx1, rg1);
        __syncthreads();
    }

    // fragment addresses inside a stage buffer: x row 32 wm + l31, chunk 2c + h; G rows 8c + 4h + s, the lane's column
    const int xfrag0 = x6_den_xoff(wm * 32 + l31, h) * 4, xfrag1 = x6_den_xoff(wm * 32 + l31, 2 + h) * 4;
    const int gfrag = XS + ((4 * h) * 256 + wn * 64 + l31) * 4;
    const int tq = l31 & 3, col0 = l31 & ~3;

    auto pass = [&](auto i_tag) {
        constexpr int i = decltype(i_tag)::value;
        f32x16 den[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) den[j][r] = 0.0f;
        for (int kb = 0; kb < nkd; ++kb) {
            const char* s = smem + b0;
            auto frags = [&](int xoff, int c, f32x4& fa, f32x4 (&fb)[2]) {
                fa = *reinterpret_cast<const f32x4*>(s + xoff);
                const float* g = reinterpret_cast<const float*>(s + gfrag) + c * 8 * 256;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int st = 0; st < 4; ++st) fb[j][st] = g[st * 256 + j * 32];
            };
            auto mfmas = [&](const f32x4& fa, const f32x4 (&fb)[2]) {
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        den[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st], fb[j][st], den[j], 0, 0, 0);
            };
            f32x4 fa, fb[2];
            frags(xfrag0, 0, fa, fb);
            mfmas(fa, fb);
            __builtin_amdgcn_sched_barrier(0);
            lstore(b2, rx, rg);
            f32x4 ga, gb[2];
            frags(xfrag1, 1, ga, gb);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);
            gload(rx, rg);
            mfmas(ga, gb);
            __builtin_amdgcn_sched_barrier(0);
            const int t0 = b0;
            b0 = b1;
            b1 = b2;
            b2 = t0;
        }
        // quotient of this pass's 128 rows: 4 x 4 transposes inside the lane quads, 16 bytes per lane
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 a, d;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = num[i][j][4 * g + e];
                    d[e] = den[j][4 * g + e];
                }
                epi.quot4(m0 + wm * 64 + i * 32 + 8 * g + 4 * h + tq, n0 + wn * 64 + j * 32 + col0,
                          quad_transpose(a, tq), quad_transpose(d, tq));
            }
    };
    pass(std::integral_constant<int, 0>{});
    pass(std::integral_constant<int, 1>{});
}

template <class Cfg, int ALAY, int BLAY, class Epi>
__global__ void __launch_bounds__(Cfg::NTHREADS, Cfg::MINW) gemm_bf16x6_kernel(GemmProblem p, Epi epi) {
    constexpr int BM = Cfg::BM, BN = Cfg::BN, BK = Cfg::BK, WM = Cfg::WM, WN = Cfg::WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int NT = Cfg::NTHREADS;
    constexpr int GA = BM * BK / 4 / NT, GB = BN * BK / 4 / NT;
    constexpr int PA = X6Panel<BM>::PLANE_BYTES, PB = X6Panel<BN>::PLANE_BYTES;
    constexpr int BUF = X6Panel<BM>::BYTES + X6Panel<BN>::BYTES;   // one buffer: A planes, then B planes
    static_assert(epi_mode<Epi>::value == 0 && !epi_rowbits<Epi>::value, "bf16x6 core: plain real epilogues");

    extern __shared__ __attribute__((aligned(16))) char x6_smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, h = lane >> 5;

    // ---- tile decode: as gemm_mfma_kernel (XCD aware, two-segment B, split-K) ----
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = p.tiles_m * p.tiles_n;
    const int split = lid / tiles;
    const int t = lid - split * tiles;
    int mt, nt;
    if (p.mt_fast) {
        mt = t % p.tiles_m;
        nt = t / p.tiles_m;
    } else {
        nt = t % p.tiles_n;
        mt = t / p.tiles_n;
    }
    const int m0 = mt * BM;
    const int kbeg = split * p.klen;
    const int kend = min(p.K, kbeg + p.klen);
    const float* Bp = p.B;
    long ldb = p.ldb;
    int nB0 = nt * BN;
    int n0 = nB0;
    if (nt >= p.tiles_n1) {
        Bp = p.B2;
        ldb = p.ldb2;
        nB0 = (nt - p.tiles_n1) * BN;
        n0 = p.n_b1 + nB0;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // Pipeline, STAGES == 2 (one barrier per K block, at the block boundary): on entry to block kb, buffer
    // kb & 1 holds block kb's planes and ra / rb hold block kb + 1's fp32 values.  Block kb's MFMAs run in two
    // groups of 6 TN, one per 32-row A block; the split and the ds_writes of block kb + 1's A panel follow the
    // first 2 TN MFMAs of the first group, those of its B panel the first 2 TN of the second, each followed by
    // that panel's loads for block kb + 2.  The other buffer was last read in block kb - 1, before the barrier
    // that ended it, so it may be written now.  The loads of the last block re-read block nkb - 1 (in bounds;
    // never used), which keeps the interior branch free.
    //
    // Pipeline, STAGES == 3 (one barrier per K block, inside the block): on entry to block kb, buffer kb % 3
    // holds block kb, buffer (kb + 1) % 3 holds block kb + 1 (complete) and ra / rb hold block kb + 2's fp32
    // values.  During block kb a wave stages block kb + 2 into buffer (kb + 2) % 3 at the same two places and
    // issues the loads of block kb + 3 behind each store.  The barrier B(kb) sits after the wave's last
    // fragment read of block kb (the second group's fa[h], read behind the first group's last product) and the
    // second group's first product, before that group's B-panel staging and before any read of block kb + 1
    // (which the second group issues as its planes die: see the fragment registers below).  The waves of a SIMD
    // cross the block boundary staggered by the matrix pipe and one wave's fragment reads run under the others'
    // MFMAs.  Why one barrier is enough:
    //   - a buffer is overwritten only after a barrier that follows every wave's reads of it: buffer
    //     (kb + 2) % 3 = (kb - 1) % 3 was last read in block kb - 1, all of those reads precede B(kb - 1), and
    //     both stagings of block kb follow B(kb - 1);
    //   - a buffer is read only after a barrier that follows every wave's writes of it: block kb + 2 is read
    //     after B(kb + 1), and both stagings of block kb precede B(kb + 1).
    // (With two buffers the second condition fails for the B panel: hence the boundary barrier above.)
    // The prologue stores blocks 0 and 1 and loads block 2 (clamped to nkb - 1: a short product re-reads its
    // last block into a buffer nobody reads).  The last two blocks are peeled: block nkb - 2 stages nothing but
    // keeps its barrier (block nkb - 1's B panel was written after B(nkb - 3)); block nkb - 1 has neither.  The
    // tail therefore writes no LDS at all, and the last staged block nkb - 3 writes buffer (nkb - 1) % 3, which
    // nobody has read since B(nkb - 4).
    static_assert(TM == 2, "one panel's staging per 32-row A block");
    constexpr int STAGES = Cfg::STAGES;
    static_assert(STAGES == 2 || STAGES == 3, "two buffers and a boundary barrier, or a ring of three");
    constexpr bool REFILL = STAGES == 3;   // fragment registers refilled as their planes die (below)
    f32x4 ra[GA], rb[GB];
    const int nkb = (kend - kbeg) / BK;   // whole K blocks (x6_eligible)
    if (nkb > 0) {
        x6_gload<ALAY, BM, NT, REFILL>(ra, p.A, p.lda, m0, kbeg, tid);
        x6_gload<BLAY, BN, NT, REFILL>(rb, Bp, ldb, nB0, kbeg, tid);
        x6_lds_store<ALAY, BM, NT>(x6_smem, ra, tid);
        x6_lds_store<BLAY, BN, NT>(x6_smem + X6Panel<BM>::BYTES, rb, tid);
        const int k1 = kbeg + min(1, nkb - 1) * BK;
        x6_gload<ALAY, BM, NT, REFILL>(ra, p.A, p.lda, m0, k1, tid);
        x6_gload<BLAY, BN, NT, REFILL>(rb, Bp, ldb, nB0, k1, tid);
        if constexpr (STAGES == 3) {
            x6_lds_store<ALAY, BM, NT>(x6_smem + BUF, ra, tid);
            x6_lds_store<BLAY, BN, NT>(x6_smem + BUF + X6Panel<BM>::BYTES, rb, tid);
            const int k2 = kbeg + min(2, nkb - 1) * BK;
            x6_gload<ALAY, BM, NT, REFILL>(ra, p.A, p.lda, m0, k2, tid);
            x6_gload<BLAY, BN, NT, REFILL>(rb, Bp, ldb, nB0, k2, tid);
        }
    }
    __syncthreads();

    // fragment byte offsets inside a plane (the same for every K block and buffer)
    static_assert(WM == 64 && WN == 64 && TN == 2, "x6_frag_next32: two 32-row blocks per 64-row wave tile");
    const int aoff = x6_frag_off<ALAY, BM>(wm * WM, lane), boff = x6_frag_off<BLAY, BN>(wn * WN, lane);
    // (the two-buffer loop keeps one offset per 32-row block, as it always had)
    int aoff2[TM], boff2[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aoff2[i] = REFILL ? 0 : x6_frag_off<ALAY, BM>(wm * WM + i * 32, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) boff2[j] = REFILL ? 0 : x6_frag_off<BLAY, BN>(wn * WN + j * 32, lane);

    // products (of six) that go out before a group's staging
    constexpr int STAGE_AFTER = 2;
    // small terms first, hh last; plane index 0 = h, 1 = m, 2 = l
    constexpr int TA[6] = {2, 0, 1, 1, 0, 0};
    constexpr int TB[6] = {0, 2, 1, 0, 1, 0};
    // Fragment registers.  The term order lets them die one plane at a time: within a group fa[l] is dead after
    // product 0, fa[m] after product 3, fa[h] after product 5; fb serves both groups and in the second one fb[l]
    // is dead after product 1, fb[m] after product 4, fb[h] after product 5.
    //   STAGES == 2: a block reads fb at its start and fa at the start of each group, as the boundary barrier
    //     demands.
    //   STAGES == 3 (REFILL): a dead plane's registers take at once the next fragment that will live in them, so
    //     only MFMAs lie between most fragment reads and their use, and no registers are added (the assignment
    //     goes to the old array element and sched barriers pin each read behind the last MFMA that reads its
    //     destination).  Group 0 of block kb reads group 1's A fragments; group 1, after B(kb), reads block
    //     kb + 1's fragments from buffer (kb + 1) % 3 (NEXT), so a block starts with only the h reads outstanding.
    //     B(kb) sits behind group 1's first product (fa[l] . fb[h]), which runs while fa[h] lands.  The ring's two
    //     conditions hold for this position:
    //       - it follows the wave's last fragment read of block kb (group 1's fa[h], read after group 0's last
    //         product), so buffer kb % 3 is overwritten (the stagings of block kb + 1) only after every read of it;
    //       - it precedes block kb's B-panel staging and every read of block kb + 1.  Block kb + 1's A panel was
    //         staged before B(kb - 1) and its B panel before B(kb) (blocks 0 and 1: before the prologue's barrier),
    //         so all of its reads follow its writes; all of them still precede B(kb + 1), after which the stagings
    //         of block kb + 2 overwrite that buffer.
    //     The prologue reads block 0's fragments; block nkb - 2 reads block nkb - 1's, block nkb - 1 none.
    x6_bf16x8 fa[3], fb[3][TN];
    // plane pl of the A fragment at byte offset off (buffer and 32-row block included), of the B fragment of
    // 32-column block j of the buffer whose first B fragment is at off
    auto afrag = [&](int off, int pl) { return x6_frag<ALAY, BM>(x6_smem + pl * PA, off); };
    auto bfrag = [&](int off, int pl, int j) {
        return x6_frag<BLAY, BN>(x6_smem + X6Panel<BM>::BYTES + pl * PB, j ? x6_frag_next32<BLAY>(off) : off);
    };
    // a buffer's first fragment offset, formed where it is used: the empty asm keeps hipcc from carrying the sums
    // of x6_smem with aoff and boff through the loop beside aoff and boff themselves (the ring has no registers
    // for that)
    auto ring_off = [](int buf, int off) {
        int o = buf + off;
        asm("" : "+v"(o));
        return o;
    };
#ifdef DCP_X6_STAMPS
    unsigned long long st_t0 = 0, st_t1 = 0, st_t2 = 0, st_t3 = 0, st_a = 0, st_b = 0, st_first = 0, st_last = 0;
    unsigned long long st_cost = 0;
    unsigned st_n = 0;
    X6_STAMP(st_t1);
    X6_STAMP(st_t0);
    st_cost = st_t0 - st_t1;
#endif
    if constexpr (REFILL) {
        // in the order of a block's refills, h last and fb[h] before fa[h], so that the loop's first wait is the
        // same count from the prologue and from the previous block
#pragma unroll
        for (int pl = 2; pl >= 0; --pl) {
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[pl][j] = bfrag(boff, pl, j);
            fa[pl] = afrag(aoff, pl);
        }
    }
    // One K block: fragments from the buffer at byte offset cur; with STAGE, ra / rb are split and stored into
    // the buffer at nxt and refilled from K offset knext; with BAR, the block has its barrier B(kb) (the ring of
    // three; the two-buffer loop puts its barrier after the block); with NEXT, group 1 reads the next block's
    // fragments from the buffer at nb.
    auto kblock = [&](int cur, int nxt_off, int knext, int nb, auto stage_tag, auto bar_tag, auto next_tag) {
        constexpr bool STAGE = decltype(stage_tag)::value;
        constexpr bool BAR = decltype(bar_tag)::value;
        constexpr bool NEXT = decltype(next_tag)::value;
        static_assert(REFILL || (!BAR && !NEXT), "the barrier inside the block and the early reads need the ring");
        char* nxt = x6_smem + nxt_off;
#ifdef DCP_X6_STAMPS
        if constexpr (BAR) {
            // st_t0: the previous block's last MFMA (or the prologue); here the first MFMA has its operands
            X6_STAMP(st_t1);
            st_a += st_t1 - st_t0;
            if (st_n == 0) st_first = st_t0;
            st_last = st_t0;
            ++st_n;
        }
#endif
        if constexpr (!REFILL) {
            // B fragments of the block first, then the A fragments of one 32-row block at a time: at four waves
            // per SIMD (128 VGPRs) all of them at once would spill
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    fb[pl][j] = x6_frag<BLAY, BN>(x6_smem + cur + X6Panel<BM>::BYTES + pl * PB, boff2[j]);
        }
        auto group = [&](auto i_tag) {
            constexpr int i = decltype(i_tag)::value;
            if constexpr (!REFILL) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) fa[pl] = x6_frag<ALAY, BM>(x6_smem + cur + pl * PA, aoff2[i]);
            }
            int roa = 0, rob = 0;   // where this group's refills read
            if constexpr (REFILL && i == 0) roa = x6_frag_next32<ALAY>(ring_off(cur, aoff));
            if constexpr (REFILL && i == 1 && NEXT) {
                roa = ring_off(nb, aoff);
                rob = ring_off(nb, boff);
            }
            auto mfmas = [&](int t0, int t1) {
#pragma unroll
                for (int tt = t0; tt < t1; ++tt)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] =
                            __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[TA[tt]], fb[TB[tt]][j], acc[i][j], 0, 0, 0);
            };
            // plane pl of A is dead: group 0 takes group 1's fragment of this block, group 1 the next block's
            auto refill_a = [&](int pl) {
                if constexpr (i == 0 || NEXT) fa[pl] = afrag(roa, pl);
            };
            // plane pl of B is dead (second group only)
            auto refill_b = [&](int pl) {
                if constexpr (i == 1 && NEXT) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) fb[pl][j] = bfrag(rob, pl, j);
                }
            };
            mfmas(0, 1);
            if constexpr (REFILL) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (BAR && i == 1) {
                    // B(kb): every fragment of the block is on its way to registers; hipcc moves MFMAs across a
                    // barrier that nothing pins
                    __syncthreads();
                    __builtin_amdgcn_sched_barrier(0);
#ifdef DCP_X6_STAMPS
                    X6_STAMP(st_t3);
                    st_b += st_t3 - st_t2;
#endif
                }
                refill_a(2);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfmas(1, STAGE_AFTER);
            if constexpr (REFILL) {
                __builtin_amdgcn_sched_barrier(0);
                refill_b(2);
            }
            if constexpr (STAGE) {
                // the first products are out; now this wave splits and stores one panel of the block to stage
                // and issues that panel's next loads while they (and the other waves' MFMAs) run; the sched
                // barriers keep hipcc from sinking the staging to the end of the group
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (i == 0) {
                    x6_lds_store<ALAY, BM, NT>(nxt, ra, tid);
                    x6_gload<ALAY, BM, NT, REFILL>(ra, p.A, p.lda, m0, knext, tid);
                } else {
                    x6_lds_store<BLAY, BN, NT>(nxt + X6Panel<BM>::BYTES, rb, tid);
                    x6_gload<BLAY, BN, NT, REFILL>(rb, Bp, ldb, nB0, knext, tid);
                }
            }
            if constexpr (REFILL || STAGE) __builtin_amdgcn_sched_barrier(0);
            if constexpr (REFILL) {
                mfmas(STAGE_AFTER, 4);
                __builtin_amdgcn_sched_barrier(0);
                refill_a(1);
                __builtin_amdgcn_sched_barrier(0);
                mfmas(4, 5);
                __builtin_amdgcn_sched_barrier(0);
                refill_b(1);
                __builtin_amdgcn_sched_barrier(0);
                mfmas(5, 6);
#ifdef DCP_X6_STAMPS
                if constexpr (BAR && i == 0) X6_STAMP(st_t2);
                if constexpr (BAR && i == 1) X6_STAMP(st_t0);
#endif
                __builtin_amdgcn_sched_barrier(0);
                // fb[h] first: the next block's first product reads it, fa[h] only its second
                refill_b(0);
                refill_a(0);
            } else {
                mfmas(STAGE_AFTER, 6);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        group(std::integral_constant<int, 0>{});
        group(std::integral_constant<int, 1>{});
    };
    if constexpr (STAGES == 2) {
        for (int kb = 0; kb + 1 < nkb; ++kb) {
            const int cur = (kb & 1) * BUF;
            kblock(cur, cur ^ BUF, kbeg + min(kb + 2, nkb - 1) * BK, 0, std::true_type{}, std::false_type{},
                   std::false_type{});
            __syncthreads();
        }
        if (nkb > 0)
            kblock(((nkb - 1) & 1) * BUF, 0, 0, 0, std::false_type{}, std::false_type{}, std::false_type{});
    } else {
        int b0 = 0, b1 = BUF, b2 = 2 * BUF;   // byte offsets of the buffers of blocks kb, kb + 1, kb + 2
        for (int kb = 0; kb + 2 < nkb; ++kb) {
            kblock(b0, b2, kbeg + min(kb + 3, nkb - 1) * BK, b1, std::true_type{}, std::true_type{},
                   std::true_type{});
            const int t0 = b0;
            b0 = b1;
            b1 = b2;
            b2 = t0;
        }
        if (nkb > 1) kblock(b0, 0, 0, b1, std::false_type{}, std::true_type{}, std::true_type{});
        if (nkb > 0) kblock(nkb > 1 ? b1 : b0, 0, 0, 0, std::false_type{}, std::false_type{}, std::false_type{});
    }

#ifdef DCP_X6_STAMPS
    if (blockIdx.x == 0 && lane == 0) {
        unsigned long long* o = x6_stamp_buf + wave * 8;
        o[0] = st_a;
        o[1] = st_b;
        o[2] = st_last - st_first;
        o[3] = st_n;
        o[4] = st_cost;
    }
#endif

    // ---- epilogue: the 32x32x16 bf16 MFMA has the C layout of the fp32 one:
    //      col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----
    if constexpr (epi_den_tail<Epi>::value) {
        // acc is the quotient's numerator; the denominator is formed here (x6_den_tail), unsplit products only
        static_assert(BM == 256 && BN == 256 && NT == 1024 && STAGES == 3 && ALAY == KMAJOR && BLAY == KMAJOR,
                      "the denominator tail is laid out for the 256 x 256 NT tile");
        x6_den_tail(acc, epi, x6_smem, m0, n0, tid);
    } else if constexpr (epi_vec4<Epi>::value) {
        // functors with a 16-byte form always use it here (x6_epi_ok): the per-element form of a loading
        // epilogue (EpiMuNum) would be compiled beside it and spill at four waves per SIMD
        const int tq = l31 & 3, col0 = (l31 & ~3);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 x;
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = acc[i][j][4 * g + e];
                    const f32x4 y = quad_transpose(x, tq);
                    epi.vec4(m0 + wm * WM + i * 32 + 8 * g + 4 * h + tq, n0 + wn * WN + j * 32 + col0, y, split);
                }
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + wn * WN + j * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    epi(row, col, acc[i][j][r], split);
                }
            }
    }
}

// the epilogue functor's 16-byte form, when it has one, must be usable (aligned arrays, leading dims % 4 == 0)
template <class Epi>
inline bool x6_epi_ok(const Epi& epi) {
    if constexpr (epi_vec4<Epi>::value) return epi.vec_ok();
    else return true;
}

// Whole tiles, whole 16-deep K blocks in every split, 16-byte aligned operands with leading dims % 4 == 0
// (both forms load 16 bytes: 4 k of one row or 4 rows at one k), no stacked A.  The ring of three also wants a
// thread's part of a panel address in 32 bits (x6_gload, SBASE): under `rows` rows of ld floats in a KMAJOR panel
// (ld under about 4 Mi floats on the 256 x 256 tile), under 16 k rows in an XMAJOR one (ld under about 68 Mi floats).  A
// product with a longer leading dimension used to run here and now takes what its caller does without this core:
// x6_tier() falls to the 128 x 128 tile, which has no such bound, or to X6_NONE (the fp32 core, other last bits).
template <class Cfg, int ALAY, int BLAY>
inline bool x6_eligible(const GemmProblem& p) {
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const int n1 = p.B2 != nullptr ? p.n_b1 : p.N;
    bool ok = p.M > 0 && p.N > 0 && p.K > 0 && (p.M % Cfg::BM) == 0 && (n1 % Cfg::BN) == 0 &&
              ((p.N - n1) % Cfg::BN) == 0 && (p.K % 16) == 0 && p.A2 == nullptr && (p.lda % 4) == 0 &&
              (p.ldb % 4) == 0 && al16(p.A) && al16(p.B);
    auto off32 = [](int lay, int rows, long ld) {
        return Cfg::STAGES != 3 || ((lay == KMAJOR ? (rows - 1) * ld + 16 : 15 * ld + rows) * 4 < (1L << 32));
    };
    ok = ok && off32(ALAY, Cfg::BM, p.lda) && off32(BLAY, Cfg::BN, p.ldb);
    if (p.B2 != nullptr) ok = ok && (p.ldb2 % 4) == 0 && al16(p.B2) && off32(BLAY, Cfg::BN, p.ldb2);
    if (p.ksplits > 1) ok = ok && (p.klen % 16) == 0 && p.klen > 0;
    return ok;
}

// Host launch.  Returns hipErrorInvalidValue when the problem is not eligible (callers check first).
template <class Cfg, int ALAY, int BLAY, class Epi>
inline hipError_t launch_gemm_bf16x6(hipStream_t stream, GemmProblem p, const Epi& epi) {
    if (!x6_eligible<Cfg, ALAY, BLAY>(p) || !x6_epi_ok(epi)) return hipErrorInvalidValue;
    if constexpr (epi_den_tail<Epi>::value) {
        // the tail takes the whole numerator: one split, one B segment; whole 16-deep K blocks of x.G.  The tail's
        // clamped loads would work from one K block per pass upward; 48 keeps the three stages of its prologue
        // distinct, which is all that has been tested (the NMF dispatch only sends multiples of 256)
        if (p.ksplits > 1 || p.B2 != nullptr || epi.depth < 48 || (epi.depth % 16) != 0) return hipErrorInvalidValue;
    }
    if (p.B2 == nullptr) p.n_b1 = p.N;
    p.m_a1 = p.M;
    p.tiles_m1 = p.tiles_m = p.M / Cfg::BM;
    p.tiles_n1 = p.n_b1 / Cfg::BN;
    p.tiles_n = p.tiles_n1 + (p.N - p.n_b1) / Cfg::BN;
    if (p.ksplits < 1) p.ksplits = 1;
    if (p.ksplits == 1) p.klen = p.K;
    p.vec_epi = epi_vec4<Epi>::value ? 1 : 0;
    p.al_mask = 0;
    const int grid = p.tiles_m * p.tiles_n * p.ksplits;
    if (grid <= 0) return hipSuccess;
    constexpr int lds_bytes = Cfg::STAGES * (X6Panel<Cfg::BM>::BYTES + X6Panel<Cfg::BN>::BYTES);
    const void* fn = reinterpret_cast<const void*>(&gemm_bf16x6_kernel<Cfg, ALAY, BLAY, Epi>);
    if constexpr (lds_bytes > 65536) {
        static DynLdsRaised raised;   // per instantiation
        std::atomic<bool>& done = raised.on_current_device();
        if (!done) {
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
            if (e != hipSuccess) return e;
            done = true;
        }
    }
    hipLaunchKernelGGL((gemm_bf16x6_kernel<Cfg, ALAY, BLAY, Epi>), dim3(grid), dim3(Cfg::NTHREADS), lds_bytes,
                       stream, p, epi);
    return hipGetLastError();
}

}  // namespace dcp
