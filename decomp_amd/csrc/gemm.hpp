// One GEMM front end for every dtype.  gemm_route() decides once, on the host, which core runs a
// product (fp32 MFMA, gemm_mfma_f32.hpp; fp64 MFMA, gemm_mfma_f64.hpp; generic LDS-tiled VALU,
// gemm_generic.hpp), under which real image a complex product runs, the dimensions the core sees
// and the tile that is launched.  gemm() launches what the route says, plan_splits() counts tiles
// by it.  Epilogue functors (epilogue.hpp) fuse the per-element update rules of the solvers into the
// GEMM that produces their last operand.
#pragma once
#include <type_traits>

#include "epilogue.hpp"
#include "gemm_generic.hpp"
#include "gemm_mfma_bf16x6.hpp"
#include "gemm_mfma_f32.hpp"
#include "gemm_mfma_f64.hpp"
#include "reduce.hpp"
#include "scalar.hpp"

namespace dcp {

// Storage forms (all row-major, as the reference's NumPy arrays):
//   NT: C[M,N] = A[M,K] . B[N,K]^T(H)      NN: C[M,N] = A[M,K] . B[K,N]
//   TN: C[M,N] = A[K,M]^T(H) . B[K,N]
enum GemmForm { FORM_NT = 0, FORM_NN = 1, FORM_TN = 2 };
enum TileSel { TILE_AUTO = 0, TILE_LARGE = 1, TILE_SMALL = 2, TILE_HUGE = 3, TILE_SMALL_DEEP = 4, TILE_MID = 5 };

template <class T>
struct GemmArgs {
    const T* A = nullptr;
    long lda = 0;
    const T* B = nullptr;
    long ldb = 0;
    const T* B2 = nullptr;  // optional second column segment of B (columns >= n_b1)
    long ldb2 = 0;
    int n_b1 = 0;
    const T* A2 = nullptr;  // optional second ROW segment of A (rows >= m_a1); float32 MFMA core only
    long lda2 = 0;
    int m_a1 = 0;
    int M = 0, N = 0, K = 0;
    int ksplits = 1;  // >1: split the reduction; the epilogue sees the split index
    int klen = 0;     // reduction length per split (set by plan_splits)
    bool conjA = false, conjB = false;  // complex only
    int tile = TILE_AUTO;
    bool split_planned = false;  // set by plan_splits: tile tiers may count on split-K
    // complex only: scratch for the real "extended" image of B (4 * rows(B) * cols(B) reals).
    // With it NT / NN products run on the fp32 / fp64 MFMA core; TN needs none.  Null -> generic core.
    real_t<T>* ext_ws = nullptr;
    // complex only: ext_ws ALREADY holds the extended image of this B (same B, same form family) from an
    // earlier product of the caller -- the ten ISTA iterations of a solve multiply by the same A A^H
    bool ext_ready = false;
    // complex64 NN only: the planar-rows image of A ([2M, K] reals, leading dim lda_rows) when the caller
    // already holds it (the atom sweep prepares its block matrices that way once per sweep)
    const real_t<T>* A_rows = nullptr;
    long lda_rows = 0;
};

// complex64 products on the fp32 MFMA core --------------------------------------------------
// ext(B) for a complex [R, C] matrix: real [2R, 2C], row 2r = (re, im) pairs (B's own memory
// image), row 2r+1 = (-im, re).  With the interleaved real view A2 of the other operand:
//   NT, C = A B^H : C_real[m][2n], [2n+1] = A2[m, :] . ext(B)[2n], [2n+1]   (K' = 2K)
//   NN, C = A B   : C_real[m][2n], [2n+1] = sum_kk A2[m][kk] ext(B)[kk][2n], [2n+1]
//   TN, C = A^H B : real views of both operands, 2x2 blocks combined in the epilogue (mode 2)
// i.e. the 4 real multiplies of every complex multiply, 8MNK flops, no operand copies except
// the small ext(B).
template <class R>
__global__ void __launch_bounds__(256) cplx_ext_kernel(const cx<R>* __restrict__ B, long rows, long cols,
                                                       long ld, R* __restrict__ out) {
    const long n = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long r = i / cols, c = i - r * cols;
        const cx<R> v = B[r * ld + c];
        R* o0 = out + (2 * r) * (2 * cols) + 2 * c;
        R* o1 = o0 + 2 * cols;
        o0[0] = v.re; o0[1] = v.im;
        o1[0] = -v.im; o1[1] = v.re;
    }
}

// Planar rows of a complex [R, C] matrix: real [2R, C], row 2r = Re A[r, :], row 2r+1 = Im A[r, :].
// With it a product A B whose LEFT operand is the small one needs no image of B at all:
//   NN, C = A B : G = rows(A) . B_real (B's own memory as [K, 2N]); the 2x2 block (rr ri; ir ii) of G gives
//   re = rr - ii, im = ri + ir in the epilogue (mode 3)
// (atom-block products [32 x K].[K x F]: the image of the F-long operand was 2/3 of their time).
template <class R>
__global__ void __launch_bounds__(256) cplx_rows_kernel(const cx<R>* __restrict__ A, long rows, long cols,
                                                        long ld, R* __restrict__ out) {
    const long n = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long r = i / cols, c = i - r * cols;
        const cx<R> v = A[r * ld + c];
        out[(2 * r) * cols + c] = v.re;
        out[(2 * r + 1) * cols + c] = v.im;
    }
}

// A complex64 functor may carry `static constexpr bool kCVec2 = true` with
//     bool cvec_ok() const                                   (host: arrays 16-byte aligned, leading dims even)
//     void cvec2(int row, int col0, f32x4 v, int split) const   (v = re, im of columns col0 and col0 + 1)
// In mode 1 the real accumulator columns 2n / 2n+1 ARE (re, im), so the core's 16-byte epilogue (epi_vec4)
// hands a lane two complex outputs of one row: all lanes active, 16 bytes per load / store, instead of
// 8 bytes on the even lanes.
template <class E, class = void>
struct epi_cvec2 { static constexpr bool value = false; };
template <class E>
struct epi_cvec2<E, decltype((void)E::kCVec2)> { static constexpr bool value = E::kCVec2; };

template <class E, class R = float>
struct CplxColEpi {   // kernel epilogue mode 1
    static constexpr int kMode = 1;
    static constexpr bool kVec4 = std::is_same<R, float>::value && epi_cvec2<E>::value;
    E e;
    __device__ __forceinline__ void pair(int r, int c, R re, R im, int s) const {
        e(r, c, cx<R>{re, im}, s);
    }
    __device__ __forceinline__ void operator()(int, int, R, int) const {}
    bool vec_ok() const {
        if constexpr (kVec4) return e.cvec_ok();
        else return false;
    }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int s) const {
        if constexpr (kVec4) e.cvec2(r, c0 >> 1, v, s);
    }
};
template <class E, class R = float>
struct CplxTnEpi {    // kernel epilogue mode 2
    static constexpr int kMode = 2;
    E e;
    __device__ __forceinline__ void pair(int r, int c, R re, R im, int s) const {
        e(r, c, cx<R>{re, im}, s);
    }
    __device__ __forceinline__ void operator()(int, int, R, int) const {}
};

template <class E, class R = float>
struct CplxNnEpi {    // kernel epilogue mode 3
    static constexpr int kMode = 3;
    E e;
    __device__ __forceinline__ void pair(int r, int c, R re, R im, int s) const {
        e(r, c, cx<R>{re, im}, s);
    }
    __device__ __forceinline__ void operator()(int, int, R, int) const {}
};

template <int FORM>
inline bool cplx_on_mfma(bool conjA, bool conjB, const void* ext_ws) {
    if (FORM == FORM_TN) return conjA && !conjB;
    if (FORM == FORM_NT) return conjB && !conjA && ext_ws != nullptr;
    return !conjA && !conjB && ext_ws != nullptr;
}

// MFMA tile tiers (BM, BN, BK, WM, WN, min waves/SIMD).  Measured on MI355X (tools/gemm_sweep.py,
// Y.D^T at 65536x4096x256): 256x256 / 16 waves 139 TF, 128x128 / 4 waves 110 TF -- the big tile
// halves the operand traffic per flop and one workgroup per CU is exactly one round.  The
// reduction-over-samples form (TN) is insensitive to the tile (131 TF either way) and keeps
// 128x128, whose 68 tiles x 15 splits fill one round of 1024 resident workgroups.
typedef TileCfg<256, 256, 16, 64, 64, 1> CfgHuge;      // 16 waves, 64 KiB LDS
typedef TileCfg<128, 128, 16, 64, 64, 2> CfgLarge;     // 4 waves, 32 KiB LDS -> 4 WG/CU
typedef TileCfg<128, 128, 64, 32, 64, 2> CfgMid;       // 8 waves of 32x64, 64-deep K blocks (128 KiB LDS): mid-size
                                                      // outputs (128..511 tiles, at most one per CU), e.g. y.A^H of
                                                      // an 8192-row minibatch, 8192 x 512 x 4096: 0.292 ms with 16-deep
                                                      // blocks, 0.275 ms with 64-deep ones (vendor BLAS: 0.263 ms)
typedef TileCfg<64, 64, 16, 32, 32, 2> CfgSmall;
typedef TileCfg<32, 128, 32, 32, 32, 2> CfgFlat;       // <= 32 output rows (x^T [Y|x] with <= 32 atoms)
typedef TileCfg<128, 32, 32, 32, 32, 2> CfgTall;       // <= 32 output columns (Y.D^T, x.G with <= 32 atoms)
typedef TileCfg<256, 256, 32, 64, 64, 1> CfgHugeDeep;   // 16 waves, 32-deep K blocks (128 KiB LDS): x^T [y|x] with >= 512
                                                      // atoms (dictionary step, 512 x 4608 x 8192, 7 splits: 0.362 -> 0.328 ms)
typedef TileCfg<128, 128, 16, 64, 64, 2, 3> CfgLargeX;       // the pair schedule (PIPE = 3) for row-contiguous panels
typedef TileCfg<256, 256, 32, 64, 64, 1, 3> CfgHugeDeepX;
typedef TileCfg<64, 64, 64, 32, 32, 1> CfgSmallDeep;   // 64 KiB LDS: latency-bound products on few CUs (64-row
                                                      // atom-block GEMMs): 4x fewer, 4x larger K blocks in flight

enum Tier { TIER_SMALL = 0, TIER_LARGE = 1, TIER_HUGE = 2, TIER_FLAT = 3, TIER_MID = 4, TIER_SMALL_DEEP = 5, TIER_TALL = 6, TIER_HUGE_DEEP = 7 };

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// The tile tier the float path uses for this problem (split-K planning needs it before the
// launch): the largest tile that still gives the chip enough workgroups, counting the splits
// a deep reduction allows.
template <int FORM>
inline int pick_tier(int M, int N, int K, int tile_sel, bool will_split, bool real32 = false) {
    if (tile_sel == TILE_SMALL) return TIER_SMALL;
    if (tile_sel == TILE_SMALL_DEEP) return TIER_SMALL_DEEP;
    if (tile_sel == TILE_LARGE) return TIER_LARGE;
    if (tile_sel == TILE_MID) return (FORM != FORM_TN && M >= 128 && N >= 128) ? TIER_MID : TIER_SMALL;
    if (tile_sel == TILE_HUGE) return FORM == FORM_TN ? TIER_LARGE : TIER_HUGE;
    // <= 64 output rows or columns (<= 64 atoms): a 128-wide tile would idle half of every MFMA and run
    // bounds-checked (Y.D^T 65536 x 64 x 4096: 0.60 ms on 128x128, 0.34 ms on 64x64; x^T Y 64 x 4160 x 65536: 1.07 -> 0.39 ms)
    // <= 32 (the usual NMF ranks): 32-wide tiles; these products are HBM bound (Y is read once per product:
    // Y.D^T 65536 x 32 x 4096 0.40 ms on 64x64, 0.22 ms = 4.9 TB/s on 128x32; x^T Y 32 x 4128 x 65536 0.53 -> 0.32 ms)
    if (M <= 32 && N > 32) return TIER_FLAT;
    if (N <= 32 && M > 32) return TIER_TALL;
    if (M <= 64 || N <= 64) return TIER_SMALL;
    long splits = will_split ? K / 512 : 1;
    if (splits < 1) splits = 1;
    if (splits > 64) splits = 64;
    // reduction over samples with a tall output (>= 512 atoms), split over the samples: the big tile with deep
    // K blocks (float32 problems only: the complex paths launch 64- or 128-wide tiles for this form)
    if (FORM == FORM_TN && real32 && will_split && M >= 512 && N >= 512 && tile_sel == TILE_AUTO) return TIER_HUGE_DEEP;
    if (FORM != FORM_TN) {
        const long wh = (long)ceil_div(M, CfgHuge::BM) * ceil_div(N, CfgHuge::BN);
        // (N in (128, 256), (384, 512), ...: the 256-wide tile covers no more columns than 128-wide tiles would:
        //  Y.D^T 65536 x 252 x 4096 1.117 -> 1.064 ms)
        const bool cols_ok = N >= 256 || ceil_div(N, CfgHuge::BN) * CfgHuge::BN == ceil_div(N, CfgLarge::BN) * CfgLarge::BN;
        if (M >= 256 && cols_ok && N > 128 && wh * splits >= 192) return TIER_HUGE;
    }
    // un-split products want at least two 4-wave workgroups per CU to hide latency
    const long wl = (long)ceil_div(M, CfgLarge::BM) * ceil_div(N, CfgLarge::BN);
    if (wl * splits >= (will_split ? 256 : 512)) return TIER_LARGE;
    // one 128x128 tile per CU or fewer: 8 waves per tile instead of 4 keep two waves on every SIMD
    // (deep reductions only: measured on y.A^H, K = 4096, +8 %; for K = 256..512 products -- x.G, the
    //  ISTA step -- the 64x64 tile with its 4x more workgroups is as fast or faster)
    if (FORM != FORM_TN && M >= 128 && N >= 128 && K >= 1024 && wl * splits >= 128) return TIER_MID;
    return TIER_SMALL;
}

// float64 (the reference's default dtype) and complex128 (on real-extended operands) tiles on the fp64 MFMA
// core.  Narrow outputs -- the usual NMF
// ranks of 8 .. 64 atoms -- get 32- and 64-wide tiles; before, anything under 128 fell to the generic VALU core
// (MU iteration 16384 x 4096, float64: k = 100 2.06 ms, k = 64 0.92, k = 32 0.84, k = 8 0.79 ms).
enum F64Tier { F64_GENERIC = 0, F64_128 = 1, F64_TALL64 = 2, F64_TALL32 = 3, F64_FLAT64 = 4, F64_FLAT32 = 5, F64_SQ64 = 6 };
typedef F64Cfg<64, 64, 32, 32, 1> F64Sq64;      // 4 waves: block Gram matrices of the atom sweep (deep reduction, split)
typedef F64Cfg<128, 64, 32, 32, 1> F64Tall64;   // 8 waves of 32 x 32
typedef F64Cfg<128, 32, 32, 32, 2> F64Tall32;   // 4 waves
typedef F64Cfg<64, 128, 32, 32, 1> F64Flat64;   // 8 waves
typedef F64Cfg<32, 128, 32, 32, 2> F64Flat32;   // 4 waves

inline int f64_tier(int M, int N, int tile_sel, int K = 1 << 30) {
    // (TILE_SMALL_DEEP -- the atom sweep's 64-row block products -- is a float32 tile choice; in double precision
    //  those products take the 64 x 128 tile here: the generic core needed 113 us for the 64 x 4096 x 512 one)
    if (tile_sel == TILE_SMALL) return F64_GENERIC;
    // the caller split a deep reduction over a small square output itself (Gram matrix D D^T, 256 x 256 x 4096 in 16
    // splits): 64 x 64 tiles give 256 workgroups where 128 x 128 tiles give 64 (37 -> 13 us)
    if (tile_sel == TILE_SMALL_DEEP && M > 64 && N > 64 && M <= 1024 && N <= 1024) return F64_SQ64;
    if (M > 64 && N > 64) {
        // few 128 x 128 tiles (the D-side products of an MU step: 256 x 4096 -> 64 tiles on 256 CUs): 64 x 64 tiles
        // put four times as many workgroups on the chip; these products are latency bound
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
        if (t128 < 96 && K <= 1024) return F64_SQ64;   // (shallow reductions only)
        // one 128-wide strip of tiles that cannot fill the chip (128 atoms, 16384 rows: 128 tiles): half-width tiles
        if (t128 < 192 && N <= 128 && M >= 256) return F64_TALL64;
        if (t128 < 192 && M <= 128 && N >= 256) return F64_FLAT64;
        return F64_128;
    }
    if (N <= 32 && M >= 128) return F64_TALL32;
    if (N <= 64 && M >= 128) return F64_TALL64;
    if (M <= 32 && N >= 128) return F64_FLAT32;
    if (M <= 64 && N >= 128) return F64_FLAT64;
    if (M > 32 && N > 32) return F64_SQ64;   // (33..64) x (33..64 or 65..127 handled above): small square outputs
    return F64_GENERIC;
}

// A/B knob of the pair schedule (TileCfg PIPE = 3): -1 = not yet read, 0 = pair schedule, 1 = plain schedule.
// Read ONCE from DCP_TN_PLAIN; dcp_debug_tn_plain() (test hook) overrides it so that one process can run both.
inline std::atomic<int>& tn_plain_flag() {
    static std::atomic<int> flag{-1};
    return flag;
}
inline bool tn_plain_schedule() {
    int v = tn_plain_flag().load(std::memory_order_relaxed);
    if (v < 0) {
        v = getenv("DCP_TN_PLAIN") != nullptr ? 1 : 0;
        tn_plain_flag().store(v, std::memory_order_relaxed);
    }
    return v != 0;
}

// ------------------------------------------------------------------ the route ----
// Every decision of the front end about one product, made once by gemm_route(): pure host arithmetic (no HIP call;
// the only global state read is tn_plain_schedule()).  gemm() launches by it, plan_splits() counts tiles by it, the
// solvers and the test hooks ask it instead of guessing.
enum GemmCore { CORE_F32 = 0, CORE_F64 = 1, CORE_GENERIC = 2 };
// real image of a complex product = the kernels' epilogue mode (see CplxColEpi / CplxTnEpi / CplxNnEpi)
enum CplxImage { IMG_NONE = 0, IMG_EXT_B = 1, IMG_TN_VIEWS = 2, IMG_ROWS_A = 3 };
// launched fp32 tiles: a Tier, or one of the two pair-schedule tiles
enum { TIER_LARGE_X = 8, TIER_HUGE_DEEP_X = 9 };

struct TileDims { int id, BM, BN, BK, WM, WN, PIPE; };
template <class Cfg>
constexpr TileDims tile_of(int id, int pipe = 0) { return {id, Cfg::BM, Cfg::BN, Cfg::BK, Cfg::WM, Cfg::WN, pipe}; }

struct GemmRoute {
    int core = CORE_GENERIC;
    // A thin complex128 product keeps its image here although the generic core builds none: callers that re-use
    // or size by the image (lasso's ext_ready, the dcp_gemm_* hook) asked by shape alone before: kept.
    int image = IMG_NONE;
    int img_rows = 0, img_cols = 0;   // the complex matrix that is imaged (B for EXT_B, A for ROWS_A)
    int M = 0, N = 0, K = 0, n1 = 0;  // the product as the launched core sees it; n1: columns of the first B segment
    int klen = 0, ksplits = 1;        // as the launched core receives them
    // PLANNING: the picked tier (a Tier on the fp32 core, an F64Tier otherwise) and what plan_splits counts by.  Where
    // `tile` differs, plan and launch differed before the route; ksplits, so the bits, hangs on the plan: kept.
    int tier = -1;
    int plan_M = 0, plan_N = 0, plan_n1 = 0, plan_bm = 64, plan_bn = 64;
    int kunit = 1;   // K blocks of 16 per K block of the planned tile (splits are whole tile blocks)
    // LAUNCH: the tile that runs (id: a Tier or TIER_*_X on the fp32 core, an F64Tier on the fp64 core)
    TileDims tile = {-1, 64, 64, 16, 0, 0, 0};   // (the generic core's)
    void plan_by(TileDims t) { plan_bm = t.BM; plan_bn = t.BN; }
};

inline TileDims f32_tile(int id) {
    switch (id) {
        case TIER_SMALL: return tile_of<CfgSmall>(id);
        case TIER_SMALL_DEEP: return tile_of<CfgSmallDeep>(id);
        case TIER_LARGE_X: return tile_of<CfgLargeX>(id, CfgLargeX::PIPE);
        case TIER_MID: return tile_of<CfgMid>(id);
        case TIER_HUGE: return tile_of<CfgHuge>(id);
        case TIER_HUGE_DEEP: return tile_of<CfgHugeDeep>(id);
        case TIER_HUGE_DEEP_X: return tile_of<CfgHugeDeepX>(id, CfgHugeDeepX::PIPE);
        case TIER_FLAT: return tile_of<CfgFlat>(id);
        case TIER_TALL: return tile_of<CfgTall>(id);
        default: return tile_of<CfgLarge>(TIER_LARGE);
    }
}
inline TileDims f64_tile(int id) {
    switch (id) {
        case F64_TALL64: return tile_of<F64Tall64>(id);
        case F64_TALL32: return tile_of<F64Tall32>(id);
        case F64_FLAT64: return tile_of<F64Flat64>(id);
        case F64_FLAT32: return tile_of<F64Flat32>(id);
        case F64_SQ64: return tile_of<F64Sq64>(id);
        default: return tile_of<F64Tile>(F64_128);
    }
}

template <int FORM, class T>
inline GemmRoute gemm_route(const GemmArgs<T>& a) {
    constexpr bool f32 = std::is_same<real_t<T>, float>::value;
    GemmRoute r;
    r.M = r.plan_M = a.M; r.N = r.plan_N = a.N; r.K = a.K;
    r.n1 = r.plan_n1 = a.B2 != nullptr ? a.n_b1 : a.N;
    r.klen = a.klen; r.ksplits = a.ksplits;
    if constexpr (scalar_traits<T>::is_complex) {
        if (!cplx_on_mfma<FORM>(a.conjA, a.conjB, a.ext_ws)) return r;
        bool rows = FORM == FORM_NN && a.M < a.N;   // the left operand is the smaller one: planar rows of A
        int t_ext = F64_GENERIC;
        if constexpr (!f32) {   // (complex128 asks f64_tier without K, float64 below with it)
            const int t_rows = f64_tier(2 * a.M, 2 * a.N, a.tile);
            rows = rows && t_rows != F64_GENERIC;
            t_ext = f64_tier(FORM == FORM_TN ? 2 * a.M : a.M, 2 * a.N, a.tile);
            r.tier = rows ? t_rows : t_ext;
        }
        r.image = FORM == FORM_TN ? IMG_TN_VIEWS : rows ? IMG_ROWS_A : IMG_EXT_B;
        if (!f32 && r.tier == F64_GENERIC) return r;
        // the real-extended product: N doubles; M under the TN views and rows(A), K under ext(B)
        r.plan_N = 2 * a.N;
        r.plan_n1 *= 2;
        if (r.image != IMG_EXT_B) r.plan_M = 2 * a.M;
        if constexpr (!f32) {
            r.plan_by(f64_tile(r.tier));
            // PLAN AND LAUNCH DISAGREE (kept): the plan counts tiles of the rows(A) product, but the launch asks
            // the ext(B) tier first and runs a thin output (30 x 50 NN) on the generic core, as the caller gave it
            if (t_ext == F64_GENERIC) return r;
            r.core = CORE_F64;
            r.tile = f64_tile(r.tier);
        }
        r.M = r.plan_M; r.N = r.plan_N;
        if (r.image == IMG_EXT_B) r.K = 2 * a.K;
        // the ext(B) and rows(A) launches take B as ONE segment (a second one is counted by the plan and then
        // dropped: kept), and an un-split reduction leaves its length to the launcher
        r.n1 = r.plan_n1;
        if (r.image != IMG_TN_VIEWS) {
            r.n1 = r.N;
            if (a.ksplits <= 1) r.klen = 0;
            const bool ext = r.image == IMG_EXT_B;
            r.img_rows = !ext ? a.M : FORM == FORM_NT ? a.N : a.K;
            r.img_cols = (!ext || FORM == FORM_NT) ? a.K : a.N;
        }
        if constexpr (f32) {
            r.core = CORE_F32;
            r.tier = pick_tier<FORM>(r.M, r.N, r.K, a.tile, a.split_planned);   // (real32 = false: kept)
            r.plan_by(f32_tile(r.tier));
            // PLAN AND LAUNCH DISAGREE (kept): complex64 launches fewer tiles than it plans by.  The 32-wide and
            // deep 64 x 64 tiers collapse to 64 x 64 (rows(A) keeps the deep one); TN runs nothing above 128 x 128,
            // rows(A) neither, ext(B) keeps 256 x 256 and the 8-wave tile (whose 64-deep K blocks the plan's
            // kunit = 1 ignores)
            const int t = r.tier;
            const bool small = t == TIER_SMALL || t == TIER_FLAT || t == TIER_TALL ||
                               (t == TIER_SMALL_DEEP && r.image != IMG_ROWS_A);
            if (small) r.tile = f32_tile(TIER_SMALL);
            else if (t == TIER_SMALL_DEEP || (r.image == IMG_EXT_B && (t == TIER_HUGE || t == TIER_MID))) r.tile = f32_tile(t);
            else r.tile = f32_tile((r.image == IMG_TN_VIEWS && !tn_plain_schedule()) ? TIER_LARGE_X : TIER_LARGE);
        }
    } else if constexpr (f32) {
        r.core = CORE_F32;
        r.tier = pick_tier<FORM>(a.M, a.N, a.K, a.tile, a.split_planned, true);
        r.plan_by(f32_tile(r.tier));
        if (r.tier == TIER_HUGE_DEEP) r.kunit = CfgHugeDeep::BK / 16;
        if (r.tier == TIER_MID) r.kunit = CfgMid::BK / 16;
        int t = r.tier;
        if (t == TIER_SMALL && a.tile == TILE_AUTO) {
            // at most one workgroup per CU: occupancy is moot and the product is a chain of
            // load -> LDS -> MFMA round trips, one per K block; 64-deep blocks make 4x fewer of them
            // (small problems: Y.D^T 2048 x 32 x 512 31 -> 10 us).  Same summation order.
            const long wgs = (long)ceil_div(a.M, 64) * ceil_div(a.N, 64) * (a.ksplits > 1 ? a.ksplits : 1);
            const int depth = a.ksplits > 1 ? a.klen : a.K;
            if (wgs <= 256 && depth >= 256 && depth % 64 == 0 && a.K % 64 == 0) t = TIER_SMALL_DEEP;
        }
        // reduction over samples, both panels row-contiguous: the pair schedule (DCP_TN_PLAIN=1: A/B knob)
        if (FORM == FORM_TN && !tn_plain_schedule()) {
            if (t == TIER_HUGE_DEEP) t = TIER_HUGE_DEEP_X;
            if (t == TIER_LARGE) t = TIER_LARGE_X;
        }
        r.tile = f32_tile(t);
    } else {
        r.tier = f64_tier(a.M, a.N, a.tile, a.K);
        if (r.tier != F64_GENERIC) {
            r.core = CORE_F64;
            r.plan_by(r.tile = f64_tile(r.tier));
        }
    }
    return r;
}

// Choose split-K so that the grid reaches ~target workgroups, each split a multiple
// of 16 deep (the MFMA K block).  Returns the number of splits; sets a.klen.
template <int FORM, class T>
inline int plan_splits(GemmArgs<T>& a, int target_wgs, int max_splits, int min_blocks = 32) {
    a.split_planned = true;
    // the product, the planned tile and the K granularity as the route has them (r.tier, not r.tile: see GemmRoute)
    const GemmRoute r = gemm_route<FORM>(a);
    const bool mfma = r.core == CORE_F32;
    const int Mx = r.plan_M, Nx = r.plan_N, Kx = r.K, n1 = r.plan_n1, bm = r.plan_bm, bn = r.plan_bn, kunit = r.kunit;
    if (mfma && FORM == FORM_TN && bm == CfgHuge::BM && target_wgs > 256) target_wgs = 256;   // one 16-wave tile per CU
    const long tiles = (long)ceil_div(Mx, bm) * (ceil_div(n1, bn) + ceil_div(Nx - n1, bn));
    const long kblocks = ceil_div(Kx > 0 ? Kx : 1, 16);   // (real-extended depth for complex64)
    // splits allowed by the reduction depth: keep every split at least 512 deep (32 K blocks)
    // so that tile prologue / slab write-out stay small against the MFMA work
    long smax = kblocks / min_blocks;
    if (smax < 1) smax = 1;
    if (smax > max_splits) smax = max_splits;
    long s = tiles > 0 ? target_wgs / tiles : 1;  // floor: stay within `target` resident slots
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    if (FORM == FORM_TN && mfma && bm == CfgLarge::BM && s == 1 && tiles > target_wgs) {
        // A grid just over a whole number of rounds of resident 128x128 workgroups (complex64 minibatch
        // statistics: 1088 tiles on 1024 slots) leaves the chip nearly empty for a whole tile's time: shorter
        // workgroups shrink that tail.  Cost model: rounds / s + 1.5 % per extra set of partial slabs; every
        // split at least 1024 deep.  Measured 1024 x 17408 x 8192: 1 split 2.63 ms, 2: 2.42, 3: 2.32, 4: 2.29, 5: 2.40.
        double best = 1e30;
        long best_s = 1;
        for (long c = 1; c <= 4 && c <= kblocks / 64 && c <= max_splits; ++c) {
            const double rounds = (double)((tiles * c + target_wgs - 1) / target_wgs);
            const double cost = rounds / (double)c + 0.015 * (double)c;
            if (cost < best - 1e-9) { best = cost; best_s = c; }
        }
        s = best_s;
    }
    long blocks_per_split = (kblocks + s - 1) / s;
    blocks_per_split = ((blocks_per_split + kunit - 1) / kunit) * kunit;
    a.klen = (int)(blocks_per_split * 16);   // in units of the core's reduction index (see gemm())
    a.ksplits = ceil_div(Kx > 0 ? Kx : 1, a.klen);
    return a.ksplits;
}

// A . B^H with a deep reduction whose 256x256 tiles alone cannot fill the chip (complex64 minibatch y.A^H:
// 8192 x 1024 x 16384 as the real core sees it -> 128 tiles): S splits on the big tile instead of the un-split
// 128x128 tile (measured 2.27 -> 1.99 ms including the ordered slab sum).  Every split stays >= 8192 deep: at
// 4096 (float32 minibatch, 64 tiles) the two plans tie.  Returns S and plans `a` for it; 1 leaves `a` untouched.
template <class T>
inline int plan_deep_nt(GemmArgs<T>& a, int max_s) {
    long Mx = a.M, Nx = a.N, Kx = a.K;
    if (std::is_same<T, c64>::value) {
        if (!cplx_on_mfma<FORM_NT>(a.conjA, a.conjB, a.ext_ws)) return 1;
        Nx *= 2; Kx *= 2;
    } else if (!std::is_same<T, float>::value) {
        return 1;
    }
    if (Mx < CfgHuge::BM || Nx < CfgHuge::BN) return 1;
    const long wh = (long)ceil_div(Mx, CfgHuge::BM) * ceil_div(Nx, CfgHuge::BN);
    if (wh >= 192) return 1;
    const long S = (256 + wh - 1) / wh;
    if (S < 2 || S > max_s || Kx / S < 8192) return 1;
    const long kblocks = (Kx + 15) / 16;
    a.tile = TILE_HUGE;
    a.klen = (int)(((kblocks + S - 1) / S) * 16);
    a.ksplits = ceil_div(Kx, a.klen);
    a.split_planned = true;
    return a.ksplits;
}

// The kernel-argument struct of the MFMA core a route names (GemmProblem / GemmProblemD), filled from the caller's
// arguments and the route.  Complex operands enter as real views (two reals per element) unless the route puts an
// image in their place: `image` is what launch_cplx_image() returned.
template <int FORM, class T>
inline auto fill_problem(const GemmArgs<T>& a, const GemmRoute& r, const real_t<T>* image = nullptr) {
    typedef real_t<T> R;
    constexpr int w = scalar_traits<T>::is_complex ? 2 : 1;
    typename std::conditional<std::is_same<R, float>::value, GemmProblem, GemmProblemD>::type p;
    p.A = reinterpret_cast<const R*>(a.A); p.lda = w * a.lda;
    p.B = reinterpret_cast<const R*>(a.B); p.ldb = w * a.ldb;
    p.B2 = reinterpret_cast<const R*>(a.B2); p.ldb2 = w * a.ldb2;
    if constexpr (std::is_same<T, float>::value) { p.A2 = a.A2; p.lda2 = a.lda2; p.m_a1 = a.m_a1; }
    if (r.image == IMG_ROWS_A) { p.A = image; p.lda = a.A_rows != nullptr ? a.lda_rows : r.img_cols; }
    if (r.image == IMG_EXT_B) { p.B = image; p.ldb = 2 * r.img_cols; }
    if (r.image == IMG_ROWS_A || r.image == IMG_EXT_B) { p.B2 = nullptr; p.ldb2 = 0; }
    p.M = r.M; p.N = r.N; p.K = r.K; p.n_b1 = r.n1;
    p.ksplits = r.ksplits; p.klen = r.klen;
    p.tiles_m = p.tiles_n = 0;
    // NT walks n tiles first (they share the A row panel); TN/NN walk m first.
    p.mt_fast = (FORM == FORM_NT) ? 0 : 1;
    return p;
}
template <int FORM, class T>
inline auto fill_problem(const GemmArgs<T>& a) {
    return fill_problem<FORM>(a, gemm_route<FORM>(a));
}

// Builds the real image the route asks for in the caller's scratch (ext(B): [2 rows, 2 cols] reals; rows(A):
// [2M, K] reals, 2MK <= 4KN) and returns it; the caller's own rows(A), or an ext(B) it declared ready, is taken
// as it is.  Null when the product needs none.
template <class T>
inline const real_t<T>* launch_cplx_image(hipStream_t stream, const GemmArgs<T>& a, const GemmRoute& r) {
    typedef real_t<T> R;
    if (r.image != IMG_ROWS_A && r.image != IMG_EXT_B) return nullptr;
    if (r.image == IMG_ROWS_A && a.A_rows != nullptr) return a.A_rows;
    long g = ((long)r.img_rows * r.img_cols + 255) / 256;
    g = g > 4096 ? 4096 : g < 1 ? 1 : g;
    if (r.image == IMG_ROWS_A)
        hipLaunchKernelGGL((cplx_rows_kernel<R>), dim3((unsigned)g), dim3(256), 0, stream, a.A, (long)r.img_rows,
                           (long)r.img_cols, a.lda, a.ext_ws);
    else if (!a.ext_ready)
        hipLaunchKernelGGL((cplx_ext_kernel<R>), dim3((unsigned)g), dim3(256), 0, stream, a.B, (long)r.img_rows,
                           (long)r.img_cols, a.ldb, a.ext_ws);
    return a.ext_ws;
}

// The one switch over the launched tile, per core.  The `if constexpr` guards name the tiles a form / image can
// be routed to (gemm_route), so that no other kernel is instantiated.
template <int FORM, int IMAGE, class Epi>
inline hipError_t launch_tile(const GemmRoute& r, hipStream_t stream, const GemmProblem& p, const Epi& epi) {
    constexpr int AL = (FORM == FORM_TN) ? XMAJOR : KMAJOR;
    constexpr int BL = (FORM == FORM_NT) ? KMAJOR : XMAJOR;
    constexpr bool real = IMAGE == IMG_NONE, pair = FORM == FORM_TN, deep64 = real || IMAGE == IMG_ROWS_A;
    constexpr bool big = FORM != FORM_TN && (real || IMAGE == IMG_EXT_B);
    switch (r.tile.id) {
        case TIER_SMALL: return launch_gemm_mfma<CfgSmall, AL, BL, Epi>(stream, p, epi);
        case TIER_LARGE: return launch_gemm_mfma<CfgLarge, AL, BL, Epi>(stream, p, epi);
        case TIER_SMALL_DEEP:
            if constexpr (deep64) return launch_gemm_mfma<CfgSmallDeep, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_LARGE_X:
            if constexpr (pair) return launch_gemm_mfma<CfgLargeX, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_HUGE_DEEP_X:
            if constexpr (pair && real) return launch_gemm_mfma<CfgHugeDeepX, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_HUGE_DEEP:
            if constexpr (real) return launch_gemm_mfma<CfgHugeDeep, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_FLAT:
            if constexpr (real) return launch_gemm_mfma<CfgFlat, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_TALL:
            if constexpr (real) return launch_gemm_mfma<CfgTall, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_HUGE:
            if constexpr (big) return launch_gemm_mfma<CfgHuge, AL, BL, Epi>(stream, p, epi); else break;
        case TIER_MID:
            if constexpr (big) return launch_gemm_mfma<CfgMid, AL, BL, Epi>(stream, p, epi); else break;
    }
    return hipErrorInvalidValue;   // (a tile the route never names for this form / image)
}
template <int FORM, int IMAGE, class Epi>
inline hipError_t launch_tile(const GemmRoute& r, hipStream_t stream, const GemmProblemD& p, const Epi& epi) {
    constexpr int AL = (FORM == FORM_TN) ? XMAJOR : KMAJOR;
    constexpr int BL = (FORM == FORM_NT) ? KMAJOR : XMAJOR;
    switch (r.tile.id) {
        case F64_TALL64: return launch_gemm_mfma_f64_cfg<F64Tall64, AL, BL, Epi>(stream, p, epi);
        case F64_TALL32: return launch_gemm_mfma_f64_cfg<F64Tall32, AL, BL, Epi>(stream, p, epi);
        case F64_FLAT64: return launch_gemm_mfma_f64_cfg<F64Flat64, AL, BL, Epi>(stream, p, epi);
        case F64_FLAT32: return launch_gemm_mfma_f64_cfg<F64Flat32, AL, BL, Epi>(stream, p, epi);
        case F64_SQ64: return launch_gemm_mfma_f64_cfg<F64Sq64, AL, BL, Epi>(stream, p, epi);
        default: return launch_gemm_mfma_f64<AL, BL, Epi>(stream, p, epi);
    }
}

template <int FORM, class T, class Epi>
inline hipError_t launch_generic(hipStream_t stream, const GemmArgs<T>& a, const GemmRoute& r, const Epi& epi) {
    GenericProblem<T> p;
    p.A = a.A; p.B = a.B; p.B2 = a.B2; p.n_b1 = a.n_b1;
    if (FORM == FORM_TN) { p.sAm = 1; p.sAk = a.lda; } else { p.sAm = a.lda; p.sAk = 1; }
    if (FORM == FORM_NT) { p.sBk = 1; p.sBn = a.ldb; p.sB2k = 1; p.sB2n = a.ldb2; }
    else { p.sBk = a.ldb; p.sBn = 1; p.sB2k = a.ldb2; p.sB2n = 1; }
    p.M = r.M; p.N = r.N; p.K = r.K;
    p.ksplits = r.ksplits; p.klen = r.klen;
    p.tiles_m = p.tiles_n = 0;
    constexpr bool cplx = scalar_traits<T>::is_complex;
    return launch_gemm_generic<T, Epi>(stream, p, cplx && a.conjA, cplx && a.conjB, epi);
}

// Take the route, build the image it asks for, launch its tile: every branch here tests a field of the route.
template <int FORM, class T, class Epi>
inline hipError_t gemm(hipStream_t stream, const GemmArgs<T>& a, const Epi& epi) {
    typedef real_t<T> R;
    const GemmRoute r = gemm_route<FORM>(a);
    if constexpr (!std::is_same<T, float>::value) {   // (float32 is never routed to the generic core)
        if (r.core == CORE_GENERIC) return launch_generic<FORM>(stream, a, r, epi);
    }
    if constexpr (!scalar_traits<T>::is_complex) {
        return launch_tile<FORM, IMG_NONE>(r, stream, fill_problem<FORM>(a, r), epi);
    } else {
        const auto p = fill_problem<FORM>(a, r, launch_cplx_image(stream, a, r));
        if constexpr (FORM == FORM_TN) {
            return launch_tile<FORM, IMG_TN_VIEWS>(r, stream, p, CplxTnEpi<Epi, R>{epi});
        } else {
            if (r.image == IMG_ROWS_A) return launch_tile<FORM, IMG_ROWS_A>(r, stream, p, CplxNnEpi<Epi, R>{epi});
            return launch_tile<FORM, IMG_EXT_B>(r, stream, p, CplxColEpi<Epi, R>{epi});
        }
    }
}

// float32 products on the split-bf16 core (gemm_mfma_bf16x6.hpp): NT (Y.D^T) and TN (x^T [Y | x]), fast path
// only.  NT takes the tile the fp32 front end would pick (256 x 256 or 128 x 128).  TN takes 256 x 256 where the
// fp32 front end picks 128 x 128, when the tiles are whole and every split is at least kX6HugeTnMinK deep (one
// 16-wave workgroup per CU: plan its splits with plan_splits_x6_tn), 128 x 128 otherwise (ragged 256-tiles,
// small shards).  x6_tier() is -1 when the problem has no bf16x6 form; gemm_bf16x6() then returns
// hipErrorInvalidValue (callers check x6_tier first).
enum { X6_NONE = -1, X6_LARGE = 0, X6_HUGE = 1 };
constexpr int kX6HugeTnMinK = 1024;

// TN on 256 x 256 by shape alone (no pointers): whole tiles in both B segments (columns < n1, >= n1) and deep
// enough splits
template <class T>
inline bool x6_huge_tn_shape(const GemmArgs<T>& a, int n1, int klen) {
    return std::is_same<T, float>::value && a.A2 == nullptr && a.M > 0 && a.N > 0 && a.K > 0 &&
           a.M % X6Huge::BM == 0 && n1 % X6Huge::BN == 0 && (a.N - n1) % X6Huge::BN == 0 && klen >= kX6HugeTnMinK &&
           pick_tier<FORM_TN>(a.M, a.N, a.K, a.tile, true, true) == TIER_LARGE;
}

// Split-K plan of a TN product that will run on the 256 x 256 bf16x6 tile: one round of 16-wave workgroups
// (one per CU, 256 CUs), every split at least 512 deep.  Returns false (and leaves `a` alone) when the product
// would not take that tile; the caller then plans for the fp32 front end (plan_splits).  n1: width of the
// first B segment (a.N without a second one).
template <class T>
inline bool plan_splits_x6_tn(GemmArgs<T>& a, int n1, int max_splits) {
    if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.M % X6Huge::BM || n1 % X6Huge::BN || (a.N - n1) % X6Huge::BN)
        return false;
    const long tiles = (long)(a.M / X6Huge::BM) * (n1 / X6Huge::BN + (a.N - n1) / X6Huge::BN);
    const long kblocks = ceil_div(a.K, 16);
    long smax = kblocks / 32;
    if (smax < 1) smax = 1;
    if (smax > max_splits) smax = max_splits;
    long s = 256 / tiles;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int klen = (int)(((kblocks + s - 1) / s) * 16);
    if (!x6_huge_tn_shape(a, n1, klen)) return false;
    a.split_planned = true;
    a.klen = klen;
    a.ksplits = ceil_div(a.K, klen);
    return true;
}

template <int FORM>
inline int x6_tier(const GemmArgs<float>& a) {
    if (FORM == FORM_NN) return X6_NONE;
    constexpr int AL = (FORM == FORM_TN) ? XMAJOR : KMAJOR, BL = (FORM == FORM_NT) ? KMAJOR : XMAJOR;
    const int tier = pick_tier<FORM>(a.M, a.N, a.K, a.tile, a.split_planned, true);
    const GemmProblem p = fill_problem<FORM>(a);
    if (FORM == FORM_NT && tier == TIER_HUGE && x6_eligible<X6Huge, AL, BL>(p)) return X6_HUGE;
    if (FORM == FORM_TN && tier == TIER_LARGE && x6_huge_tn_shape(a, a.B2 != nullptr ? a.n_b1 : a.N, a.ksplits > 1 ? a.klen : a.K) &&
        x6_eligible<X6Huge, AL, BL>(p))
        return X6_HUGE;
    if ((tier == TIER_LARGE || (FORM == FORM_NT && (tier == TIER_MID || tier == TIER_HUGE))) &&
        x6_eligible<X6Large, AL, BL>(p))
        return X6_LARGE;
    return X6_NONE;
}

template <int FORM, class Epi>
inline hipError_t gemm_bf16x6(hipStream_t stream, const GemmArgs<float>& a, const Epi& epi) {
    constexpr int AL = (FORM == FORM_TN) ? XMAJOR : KMAJOR;
    constexpr int BL = (FORM == FORM_NT) ? KMAJOR : XMAJOR;
    if constexpr (FORM == FORM_NN) {
        return hipErrorInvalidValue;
    } else {
        const int t = x6_tier<FORM>(a);
        if (t == X6_HUGE) return launch_gemm_bf16x6<X6Huge, AL, BL, Epi>(stream, fill_problem<FORM>(a), epi);
        if (t == X6_LARGE) return launch_gemm_bf16x6<X6Large, AL, BL, Epi>(stream, fill_problem<FORM>(a), epi);
        return hipErrorInvalidValue;
    }
}

}  // namespace dcp
