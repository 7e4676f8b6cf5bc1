// assemble_items.hpp — layouts, parameter blocks, robust loss, and the per-correspondence item functions of the three problems.
// Part of the hand-written gfx950 kernels of the Gauss-Newton normal-equation assembly path; see assemble_kernels.hpp
// (the umbrella header every translation unit includes) for the overview and the reference citations.
#pragma once

#include <hip/hip_runtime.h>
#include <limits>

#include "host/nos_lm.hpp"
#include <stdint.h>

// -DNOS_LM_TIMING is the probe build of tools/ (device time stamps of the phases of a launch).  Everything it adds to the
// kernels sits inside NOS_PROBE(...) or one of the three stamp macros defined from it; the product build compiles none of it.
#ifdef NOS_LM_TIMING
#define NOS_PROBE(...) __VA_ARGS__
#else
#define NOS_PROBE(...)
#endif

namespace nos {

constexpr int kWave = 64;

enum LossKind : int { kLossNone = 0, kLossExponential = 1, kLossHuber = 2 };

// Tiled SoA addressing.  Correspondence i, field f lives at element offset
//   (i >> tile_shift) * tile_stride + f * field_stride + (i & (tile - 1)).
// tile == n_padded, tile_stride == 0 gives a plain planar layout.
// Flat NDT datasets store 21 planes: the 12 the kernels stream — p (3), mu (3), U (u00 u01 u02 u11 u12 u22: S = QU,
// sqrt_info_to_U) — in
// the layout above, then the 9 planes of S (row-major) in a second region of the same allocation, laid out alike:
//   s_offset + (i >> tile_shift) * s_tile_stride + k * field_stride + (i & (tile - 1)),
// so that a pass over the streamed planes never touches S (nos_dataset_download and the fp32 3-DoF item read it).
struct TiledLayout {
  const void* base;
  uint64_t n;            // real correspondences
  uint64_t n_padded;     // multiple of tile (pads are all-zero records)
  uint64_t tile_stride;  // elements between consecutive tiles
  uint64_t field_stride; // elements between consecutive fields inside a tile
  uint32_t tile_shift;   // log2(tile)
  uint32_t tile_mask;    // tile - 1
  uint64_t s_offset;     // flat NDT: element offset of the S region
  uint64_t s_tile_stride;  // flat NDT: elements between consecutive tiles of the S region
};

constexpr int kNdtStreamed = 12;  // planes of a flat NDT dataset the kernels stream: p, mu, U
constexpr int kNdtStored = 21;    // and the 9 planes of S behind them
// stored plane of plane f of the caller's view (p, mu, S row-major: the 15 planes of nos.h)
__host__ __device__ constexpr int ndt_stored_plane(int f) { return f < 6 ? f : f + 6; }
// element offset of stored plane f (0 … 20; reprojection and voxel-indexed datasets: their own planes, all < 12) of item i
__host__ __device__ inline uint64_t plane_offset(const TiledLayout& L, uint64_t i, int f) {
  if (f < kNdtStreamed) return (i >> L.tile_shift) * L.tile_stride + uint64_t(f) * L.field_stride + (i & L.tile_mask);
  return L.s_offset + (i >> L.tile_shift) * L.s_tile_stride + uint64_t(f - kNdtStreamed) * L.field_stride + (i & L.tile_mask);
}
// U = the upper-triangular factor of a QR of a row-major sqrt-information S (S = Q U, so UᵀU = SᵀS), in the element type
// of the dataset: u00 u01 u02 u11 u12 u22.  Computed in fp64 from the stored S by three Givens rotations (backward stable:
// Q̂U = S + ΔS, ‖ΔS‖ ≈ u‖S‖; a rank-deficient S gives a zero row of U), then rounded once.  The items evaluate
// r' = U e = Qᵀ(S e), s = r'ᵀr' and J' = [U | U M] (Ndt6Problem::item_U): the error of s grows like u·κ(S), as in the
// S form of the reference, not like u·κ(S)² as that of eᵀ(SᵀS)e does.
template <typename T>
__device__ __forceinline__ void sqrt_info_to_U(const T (&S)[9], T (&U)[6]) {
  double m[3][3];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k / 3][k % 3] = double(S[k]);
  // zero (1,0) and (2,0) against row 0, then (2,1) against row 1
  const int rot[3][3] = {{0, 1, 0}, {0, 2, 0}, {1, 2, 1}};  // pivot row, zeroed row, column
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int i = rot[q][0], j = rot[q][1], c = rot[q][2];
    const double a = m[i][c], b = m[j][c];
    const double r = hypot(a, b);
    if (r > 0.0) {
      const double cs = a / r, sn = b / r;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k <= c) continue;
        const double x = m[i][k], y = m[j][k];
        m[i][k] = fma(cs, x, sn * y);
        m[j][k] = fma(cs, y, -(sn * x));
      }
      m[i][c] = r;
      m[j][c] = 0.0;
    }
  }
  U[0] = T(m[0][0]);
  U[1] = T(m[0][1]);
  U[2] = T(m[0][2]);
  U[3] = T(m[1][1]);
  U[4] = T(m[1][2]);
  U[5] = T(m[2][2]);
}

template <typename T>
struct Ndt6Params {
  T R[9];
  T t[3];
  T la, lb, lc;  // loss: (c1, c2, 2*c1*c2) | (th, th*th, 2*th)
};

template <typename T>
struct Ndt3Params {
  T R2[4];
  T t2[2];
  T la, lb, lc;
};

template <typename T>
struct ReprojParams {
  T R[9];
  T t[3];
  T inv_fx, inv_fy, cx, cy;
  T min_depth;
  T la, lb, lc;
  // Validity rules on the depth z = (R X + t)_z, set by the launcher (set_reproj_rules):
  //   scalar class (REM/..._analytic.cc:111,119-123): a correspondence with z < min_depth contributes nothing at all
  //     → thr_w = min_depth, loss_everywhere = 0;
  //   fp32 class (REM/..._analytic_simd.cc:66-92,134): the WEIGHT counts where z > 0, residual and loss are evaluated for
  //     every correspondence → thr_w = smallest positive number, loss_everywhere = 1.  (z == 0 exactly then gives the same
  //     inf / NaN as in the reference; the damped solve reports the non-finite pivot instead of returning a pose.)
  // The second rule is a uniform flag combined with the lane mask by scalar instructions: no vector-ALU cost.
  T thr_w;
  int loss_everywhere;
};
template <typename T>
inline void set_reproj_rules(ReprojParams<T>& P, bool simd_class) {
  P.thr_w = simd_class ? std::numeric_limits<T>::min() : P.min_depth;
  P.loss_everywhere = simd_class ? 1 : 0;
}

// ---------------------------------------------------------------- math helpers

template <typename T>
__device__ __forceinline__ T fast_exp(T x);
template <>
__device__ __forceinline__ double fast_exp<double>(double x) {
  return exp(x);
}
template <>
__device__ __forceinline__ float fast_exp<float>(float x) {
  return __expf(x);
}
template <typename T>
__device__ __forceinline__ T fast_sqrt(T x);
template <>
__device__ __forceinline__ double fast_sqrt<double>(double x) {
  return sqrt(x);
}
template <>
__device__ __forceinline__ float fast_sqrt<float>(float x) {
  return sqrtf(x);
}

// 1/x and 1/sqrt(x) to full fp64 accuracy from the hardware seed plus two Newton steps (~5 / ~9 instructions
// instead of the ~20-instruction IEEE divide / sqrt sequences; the reprojection kernel is fp64-ALU bound).
// Callers pass x > 0 and finite.
template <typename T>
__device__ __forceinline__ T fast_inv(T x) {
  if constexpr (sizeof(T) == 8) {
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
  } else {
    return T(1) / x;
  }
}

template <typename T>
__device__ __forceinline__ T fast_rsqrt(T x) {
  if constexpr (sizeof(T) == 8) {
    double y = __builtin_amdgcn_rsq(x);
    // y <- y + y * (0.5 - 0.5 x y^2): quadratic convergence, twice
    double h = 0.5 * y;
    double e = fma(-x * y, h, 0.5);
    y = fma(y, e, y);
    h = 0.5 * y;
    e = fma(-x * y, h, 0.5);
    return fma(y, e, y);
  } else {
    return rsqrtf(x);
  }
}

// ---- value types of the item math.  The item functions below are written once for a value type V: the element type T
// itself (one correspondence per call) or — fp32 only — a packed pair of floats (two correspondences per call: gfx950
// has v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32; measured, the packed kernels are slower than the scalar ones, so the
// pair form is a compile-time experiment only, see assemble_kernel).  Pose, loss parameters and masks stay scalar.
using float2_t = float __attribute__((ext_vector_type(2)));

template <typename V>
struct Lanes {
  static constexpr int n = 1;
  using S = V;
};
template <>
struct Lanes<float2_t> {
  static constexpr int n = 2;
  using S = float;
};

template <typename V>
__device__ __forceinline__ V splat(typename Lanes<V>::S s) {
  if constexpr (Lanes<V>::n == 2)
    return V{s, s};
  else
    return s;
}
template <typename V>
__device__ __forceinline__ V vfma(V a, V b, V c) {
  if constexpr (Lanes<V>::n == 2)
    return __builtin_elementwise_fma(a, b, c);
  else
    return fma(a, b, c);
}
// scalar coefficient (pose / intrinsics entry) times value plus value
template <typename V>
__device__ __forceinline__ V sfma(typename Lanes<V>::S a, V b, V c) {
  return vfma<V>(splat<V>(a), b, c);
}
template <typename V>
__device__ __forceinline__ typename Lanes<V>::S lane_get(const V& v, int k) {
  if constexpr (Lanes<V>::n == 2)
    return v[k];
  else
    return v;
}
template <typename V>
__device__ __forceinline__ void lane_set(V& v, int k, typename Lanes<V>::S s) {
  if constexpr (Lanes<V>::n == 2)
    v[k] = s;
  else
    v = s;
}

// loss_function.h:28-33 / :57-66 ; LOSS == 0 is the `loss_function_ == nullptr` branch.  Scalar form:
template <typename T, int LOSS>
__device__ __forceinline__ void loss_eval(T s, T la, T lb, T lc, T& rho, T& w) {
  if constexpr (LOSS == kLossExponential) {
    const T ex = fast_exp<T>(-lb * s);
    rho = la - la * ex;
    w = lc * ex;
  } else if constexpr (LOSS == kLossHuber) {
    const bool outlier = s > lb;           // lb = th^2
    const T sc = outlier ? s : T(1);
    const T ir = fast_rsqrt<T>(sc);        // 1 / |r|
    rho = outlier ? (lc * (sc * ir) - lb) : s;  // lc = 2 th ;  |r| = s / |r|
    w = outlier ? (la * ir) : T(1);
  } else {
    rho = s;
    w = T(1);
  }
}
// value form: per lane through the scalar form (the transcendental / select part is not packable anyway)
template <typename V, int LOSS>
__device__ __forceinline__ void loss_eval_v(V s, typename Lanes<V>::S la, typename Lanes<V>::S lb, typename Lanes<V>::S lc,
                                            V& rho, V& w) {
  using S = typename Lanes<V>::S;
#pragma unroll
  for (int k = 0; k < Lanes<V>::n; ++k) {
    S r1, w1;
    loss_eval<S, LOSS>(lane_get<V>(s, k), la, lb, lc, r1, w1);
    lane_set<V>(rho, k, r1);
    lane_set<V>(w, k, w1);
  }
}

// M = -R [p]x, column form of ..._analytic_simd_various.cc:677-687.
template <typename V>
__device__ __forceinline__ void minus_R_hat(const typename Lanes<V>::S (&R)[9], V px, V py, V pz, V (&M)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    M[i][0] = sfma<V>(R[3 * i + 2], py, -(splat<V>(R[3 * i + 1]) * pz));
    M[i][1] = sfma<V>(R[3 * i + 0], pz, -(splat<V>(R[3 * i + 2]) * px));
    M[i][2] = sfma<V>(R[3 * i + 1], px, -(splat<V>(R[3 * i + 0]) * py));
  }
}

// ---------------------------------------------------------------- problems

template <typename T, int LOSS>
struct Ndt6Problem {
  static constexpr int kFields = kNdtStreamed;  // planes an item reads: p, mu, U (see TiledLayout)
  static constexpr int kPlanes = 15;            // planes of a correspondence as the caller gives it (p, mu, S)
  static constexpr bool kSPlanes = false;       // reads S instead of U (Ndt3Problem<float>)
  static constexpr int kOut = 28;
  using Params = Ndt6Params<T>;
  // x = {p(3), mu(3), U (u00 u01 u02 u11 u12 u22)}; V = T (one correspondence) or float2_t (two, fp32 only).  Zero-padded
  // records have U = 0 → s = 0, H = g = 0, rho(0) = 0: no mask needed.
  template <typename V = T>
  __device__ static __forceinline__ void item(const V (&x)[kNdtStreamed], const Params& P,
                                              const bool (&)[Lanes<V>::n] /*valid*/, V (&acc)[28]) {
    const V p3[3] = {x[0], x[1], x[2]}, mu3[3] = {x[3], x[4], x[5]};
    const V U6[6] = {x[6], x[7], x[8], x[9], x[10], x[11]};
    item_U<V>(p3, mu3, U6, P, acc);
  }
  __device__ static __forceinline__ void item(const T (&x)[kNdtStreamed], const Params& P, bool valid, T (&acc)[28]) {
    const bool v1[1] = {valid};
    item<T>(x, P, v1, acc);
  }

  // The U form (flat datasets store the triangular factor U of S = QU, the voxel table of the indexed layout too).  With
  // J = [S | S M] and Qᵀ orthogonal, J' = QᵀJ = [U | U M] and r' = Qᵀr = U e give the same sums as the reference's S form:
  //   s = r'ᵀr',  g = w J'ᵀr',  H = w J'ᵀJ'
  // — ≈ 140 instead of ≈ 190 operations per correspondence, 12 instead of 15 values per flat record.  U is triangular, so
  // C = U M and the blocks of J'ᵀJ' cost 1 + 2 + 3 products per column.
  template <typename V = T>
  __device__ static __forceinline__ void item_U(const V (&p)[3], const V (&mu)[3], const V (&U)[6], const Params& P,
                                                V (&acc)[28]) {
    V e[3], r[3], M[3][3], C[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      e[i] = sfma<V>(P.R[3 * i], p[0], sfma<V>(P.R[3 * i + 1], p[1], sfma<V>(P.R[3 * i + 2], p[2], splat<V>(P.t[i])))) - mu[i];
    const V u00 = U[0], u01 = U[1], u02 = U[2], u11 = U[3], u12 = U[4], u22 = U[5];
    r[0] = vfma<V>(u00, e[0], vfma<V>(u01, e[1], u02 * e[2]));
    r[1] = vfma<V>(u11, e[1], u12 * e[2]);
    r[2] = u22 * e[2];
    const V s = vfma<V>(r[0], r[0], vfma<V>(r[1], r[1], r[2] * r[2]));
    V rho, w;
    loss_eval_v<V, LOSS>(s, P.la, P.lb, P.lc, rho, w);
    minus_R_hat<V>(P.R, p[0], p[1], p[2], M);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      C[0][b] = vfma<V>(u00, M[0][b], vfma<V>(u01, M[1][b], u02 * M[2][b]));
      C[1][b] = vfma<V>(u11, M[1][b], u12 * M[2][b]);
      C[2][b] = u22 * M[2][b];
    }
    // upper triangle, row-major: rows 0-2 = [UᵀU | UᵀC], rows 3-5 = CᵀC
    acc[0] = vfma<V>(w, u00 * u00, acc[0]);
    acc[1] = vfma<V>(w, u00 * u01, acc[1]);
    acc[2] = vfma<V>(w, u00 * u02, acc[2]);
    acc[6] = vfma<V>(w, vfma<V>(u01, u01, u11 * u11), acc[6]);
    acc[7] = vfma<V>(w, vfma<V>(u01, u02, u11 * u12), acc[7]);
    acc[11] = vfma<V>(w, vfma<V>(u02, u02, vfma<V>(u12, u12, u22 * u22)), acc[11]);
    if constexpr (sizeof(typename Lanes<V>::S) == 4) {
      // fp32: w folded into C and r' once (wC, wr), every entry that reads them a plain fma chain — 9 operations fewer;
      // fp64 keeps acc += w · (dot product): the 12 extra live values spill the voxel-indexed kernel's pipeline
      V wC[3][3], wr[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        wr[k] = w * r[k];
#pragma unroll
        for (int b = 0; b < 3; ++b) wC[k][b] = w * C[k][b];
      }
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        acc[3 + b] = vfma<V>(u00, wC[0][b], acc[3 + b]);
        acc[8 + b] = vfma<V>(u01, wC[0][b], vfma<V>(u11, wC[1][b], acc[8 + b]));
        acc[12 + b] = vfma<V>(u02, wC[0][b], vfma<V>(u12, wC[1][b], vfma<V>(u22, wC[2][b], acc[12 + b])));
      }
      int k = 15;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
          acc[k] = vfma<V>(C[0][a], wC[0][b], vfma<V>(C[1][a], wC[1][b], vfma<V>(C[2][a], wC[2][b], acc[k])));
          ++k;
        }
      acc[21] = vfma<V>(u00, wr[0], acc[21]);
      acc[22] = vfma<V>(u01, wr[0], vfma<V>(u11, wr[1], acc[22]));
      acc[23] = vfma<V>(u02, wr[0], vfma<V>(u12, wr[1], vfma<V>(u22, wr[2], acc[23])));
#pragma unroll
      for (int b = 0; b < 3; ++b)
        acc[24 + b] = vfma<V>(C[0][b], wr[0], vfma<V>(C[1][b], wr[1], vfma<V>(C[2][b], wr[2], acc[24 + b])));
    } else {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        acc[3 + b] = vfma<V>(w, u00 * C[0][b], acc[3 + b]);
        acc[8 + b] = vfma<V>(w, vfma<V>(u01, C[0][b], u11 * C[1][b]), acc[8 + b]);
        acc[12 + b] = vfma<V>(w, vfma<V>(u02, C[0][b], vfma<V>(u12, C[1][b], u22 * C[2][b])), acc[12 + b]);
      }
      int k = 15;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
          acc[k] = vfma<V>(w, vfma<V>(C[0][a], C[0][b], vfma<V>(C[1][a], C[1][b], C[2][a] * C[2][b])), acc[k]);
          ++k;
        }
      acc[21] = vfma<V>(w, u00 * r[0], acc[21]);
      acc[22] = vfma<V>(w, vfma<V>(u01, r[0], u11 * r[1]), acc[22]);
      acc[23] = vfma<V>(w, vfma<V>(u02, r[0], vfma<V>(u12, r[1], u22 * r[2])), acc[23]);
#pragma unroll
      for (int b = 0; b < 3; ++b)
        acc[24 + b] = vfma<V>(w, vfma<V>(C[0][b], r[0], vfma<V>(C[1][b], r[1], C[2][b] * r[2])), acc[24 + b]);
    }
    acc[27] += rho;
  }
};

template <typename T, int LOSS>
struct Ndt3Problem {
  // fp64: p, mu, U (item_U).  fp32 keeps the S form — p, mu and S (row-major) — and reads S from the dataset's S region:
  // its sums are pinned to the printed digit (tests/test_simd_class.py)
  static constexpr bool kSPlanes = sizeof(T) == 4;
  static constexpr int kFields = kSPlanes ? 15 : kNdtStreamed;
  static constexpr int kPlanes = 15;
  static constexpr int kOut = 10;
  using Params = Ndt3Params<T>;
  template <typename V = T>
  __device__ static __forceinline__ void item(const V (&x)[kFields], const Params& P, const bool (&)[Lanes<V>::n] /*valid*/,
                                              V (&acc)[10]) {
    if constexpr (!kSPlanes) {
      const T p3[3] = {x[0], x[1], x[2]}, mu3[3] = {x[3], x[4], x[5]};
      const T U6[6] = {x[6], x[7], x[8], x[9], x[10], x[11]};
      item_U(p3, mu3, U6, P, acc);
    } else {
      item_S<V>(x, P, acc);
    }
  }
  template <typename V>
  __device__ static __forceinline__ void item_S(const V (&x)[15], const Params& P, V (&acc)[10]) {
    V e[3], r[3], J[3][3];
    const V ux = x[0], uy = x[1];
    e[0] = sfma<V>(P.R2[0], ux, sfma<V>(P.R2[1], uy, splat<V>(P.t2[0]))) - x[3];
    e[1] = sfma<V>(P.R2[2], ux, sfma<V>(P.R2[3], uy, splat<V>(P.t2[1]))) - x[4];
    e[2] = x[2] - x[5];
    const V d0 = sfma<V>(P.R2[1], ux, -(splat<V>(P.R2[0]) * uy));
    const V d1 = sfma<V>(P.R2[3], ux, -(splat<V>(P.R2[2]) * uy));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r[a] = vfma<V>(x[6 + 3 * a], e[0], vfma<V>(x[7 + 3 * a], e[1], x[8 + 3 * a] * e[2]));
      J[a][0] = x[6 + 3 * a];
      J[a][1] = x[7 + 3 * a];
      J[a][2] = vfma<V>(x[6 + 3 * a], d0, x[7 + 3 * a] * d1);
    }
    const V s = vfma<V>(r[0], r[0], vfma<V>(r[1], r[1], r[2] * r[2]));
    V rho, w;
    loss_eval_v<V, LOSS>(s, P.la, P.lb, P.lc, rho, w);
    V wJ[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) wJ[a][c] = w * J[a][c];
    int k = 0;
#pragma unroll
    for (int row = 0; row < 3; ++row)
#pragma unroll
      for (int col = row; col < 3; ++col) {
        acc[k] = vfma<V>(wJ[0][row], J[0][col], vfma<V>(wJ[1][row], J[1][col], vfma<V>(wJ[2][row], J[2][col], acc[k])));
        ++k;
      }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      acc[6 + c] = vfma<V>(wJ[0][c], r[0], vfma<V>(wJ[1][c], r[1], vfma<V>(wJ[2][c], r[2], acc[6 + c])));
    acc[9] += rho;
  }
  __device__ static __forceinline__ void item(const T (&x)[kFields], const Params& P, bool valid, T (&acc)[10]) {
    const bool v1[1] = {valid};
    item<T>(x, P, v1, acc);
  }

  // U form (flat fp64 datasets, the voxel table of the indexed layout) with S = QU: J' = [U(:,0) U(:,1) U(:,0:2)·d] — U is
  // upper triangular, so J'(:,0) = (u00, 0, 0), J'(:,1) = (u01, u11, 0), J'(:,2) = (u00 d0 + u01 d1, u11 d1, 0) — and
  // r' = U e.
  __device__ static __forceinline__ void item_U(const T (&p)[3], const T (&mu)[3], const T (&U)[6], const Params& P,
                                                T (&acc)[10]) {
    const T ux = p[0], uy = p[1];
    T e[3];
    e[0] = fma(P.R2[0], ux, fma(P.R2[1], uy, P.t2[0])) - mu[0];
    e[1] = fma(P.R2[2], ux, fma(P.R2[3], uy, P.t2[1])) - mu[1];
    e[2] = p[2] - mu[2];
    const T d0 = fma(P.R2[1], ux, -(P.R2[0] * uy));
    const T d1 = fma(P.R2[3], ux, -(P.R2[2] * uy));
    const T u00 = U[0], u01 = U[1], u02 = U[2], u11 = U[3], u12 = U[4], u22 = U[5];
    const T r0 = fma(u00, e[0], fma(u01, e[1], u02 * e[2]));
    const T r1 = fma(u11, e[1], u12 * e[2]);
    const T r2 = u22 * e[2];
    const T s = fma(r0, r0, fma(r1, r1, r2 * r2));
    T rho, w;
    loss_eval<T, LOSS>(s, P.la, P.lb, P.lc, rho, w);
    const T c0 = fma(u00, d0, u01 * d1);
    const T c1 = u11 * d1;
    const T w00 = w * u00, w01 = w * u01, w11 = w * u11, wc0 = w * c0, wc1 = w * c1;
    acc[0] = fma(w00, u00, acc[0]);
    acc[1] = fma(w00, u01, acc[1]);
    acc[2] = fma(w00, c0, acc[2]);
    acc[3] = fma(w01, u01, fma(w11, u11, acc[3]));
    acc[4] = fma(w01, c0, fma(w11, c1, acc[4]));
    acc[5] = fma(wc0, c0, fma(wc1, c1, acc[5]));
    acc[6] = fma(w00, r0, acc[6]);
    acc[7] = fma(w01, r0, fma(w11, r1, acc[7]));
    acc[8] = fma(wc0, r0, fma(wc1, r1, acc[8]));
    acc[9] += rho;
  }
};

template <typename T, int LOSS>
struct ReprojProblem {
  static constexpr int kFields = 5;
  static constexpr int kPlanes = 5;
  static constexpr bool kSPlanes = false;
  static constexpr int kOut = 28;
  using Params = ReprojParams<T>;
  // x = {X(3), pixel(2)}; V = T or float2_t
  template <typename V = T>
  __device__ static __forceinline__ void item(const V (&x)[5], const Params& P, const bool (&valid)[Lanes<V>::n],
                                              V (&acc)[28]) {
    using S = typename Lanes<V>::S;
    V Xw[3], J[2][6], r[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      Xw[i] = sfma<V>(P.R[3 * i], x[0], sfma<V>(P.R[3 * i + 1], x[1], sfma<V>(P.R[3 * i + 2], x[2], splat<V>(P.t[i]))));
    // depth test of ..._analytic.cc:119-123; pads (valid == false) contribute nothing
    bool ok[Lanes<V>::n], okr[Lanes<V>::n];
    V iz;
#pragma unroll
    for (int k = 0; k < Lanes<V>::n; ++k) {
      const S z = lane_get<V>(Xw[2], k);
      ok[k] = valid[k] && !(z < P.thr_w);                          // the weight counts
      okr[k] = ok[k] || (valid[k] && P.loss_everywhere != 0);      // residual and loss are evaluated
      lane_set<V>(iz, k, fast_inv<S>(okr[k] ? z : S(1)));
    }
    const V iz2 = iz * iz;
    // (pixel − c) first: the difference is (nearly) exact, so fp32 keeps its digits in the residual
    r[0] = vfma<V>(Xw[0], iz, -(splat<V>(P.inv_fx) * (x[3] - splat<V>(P.cx))));
    r[1] = vfma<V>(Xw[1], iz, -(splat<V>(P.inv_fy) * (x[4] - splat<V>(P.cy))));
    const V k02 = -Xw[0] * iz2, k12 = -Xw[1] * iz2;
    J[0][0] = iz;
    J[0][1] = splat<V>(S(0));
    J[0][2] = k02;
    J[1][0] = splat<V>(S(0));
    J[1][1] = iz;
    J[1][2] = k12;
    // rotation block: row_a · (−R [X]x) = (X × u_a)ᵀ with u_a = R₀ᵀ/z + k_a2 R₂ᵀ (rows of R) — 24 operations instead
    // of the 30 that go through M = −R [X]x
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const V ka = a == 0 ? k02 : k12;
      V u[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) u[j] = sfma<V>(P.R[3 * a + j], iz, splat<V>(P.R[6 + j]) * ka);
      J[a][3] = vfma<V>(x[1], u[2], -(x[2] * u[1]));
      J[a][4] = vfma<V>(x[2], u[0], -(x[0] * u[2]));
      J[a][5] = vfma<V>(x[0], u[1], -(x[1] * u[0]));
    }
    V s = vfma<V>(r[0], r[0], r[1] * r[1]);
#pragma unroll
    for (int k = 0; k < Lanes<V>::n; ++k)
      if (!okr[k]) lane_set<V>(s, k, S(0));
    V rho, w;
    loss_eval_v<V, LOSS>(s, P.la, P.lb, P.lc, rho, w);
#pragma unroll
    for (int k = 0; k < Lanes<V>::n; ++k)
    {
      if (!ok[k]) lane_set<V>(w, k, S(0));
      if (!okr[k]) lane_set<V>(rho, k, S(0));
    }
    // acc += w JᵀJ (upper), w Jᵀr with the structure of this Jacobian spelled out — row 0 = [a 0 c d0 d1 d2],
    // row 1 = [0 a e f0 f1 f2] (a = 1/z): 49 operations instead of the 66 of the generic 2x6 update (the kernel is
    // fp64-VALU bound when the data is resident)
    {
      const V a = J[0][0], c = J[0][2], e = J[1][2];
      const V wa = w * a, wc = w * c, we = w * e;
      V wd[3], wf[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        wd[b] = w * J[0][3 + b];
        wf[b] = w * J[1][3 + b];
      }
      acc[0] = vfma<V>(wa, a, acc[0]);
      acc[2] = vfma<V>(wa, c, acc[2]);
      acc[6] = vfma<V>(wa, a, acc[6]);
      acc[7] = vfma<V>(wa, e, acc[7]);
      acc[11] = vfma<V>(wc, c, vfma<V>(we, e, acc[11]));
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        acc[3 + b] = vfma<V>(wa, J[0][3 + b], acc[3 + b]);
        acc[8 + b] = vfma<V>(wa, J[1][3 + b], acc[8 + b]);
        acc[12 + b] = vfma<V>(wc, J[0][3 + b], vfma<V>(we, J[1][3 + b], acc[12 + b]));
      }
      int k = 15;
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = p; q < 3; ++q) {
          acc[k] = vfma<V>(wd[p], J[0][3 + q], vfma<V>(wf[p], J[1][3 + q], acc[k]));
          ++k;
        }
      acc[21] = vfma<V>(wa, r[0], acc[21]);
      acc[22] = vfma<V>(wa, r[1], acc[22]);
      acc[23] = vfma<V>(wc, r[0], vfma<V>(we, r[1], acc[23]));
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[24 + b] = vfma<V>(wd[b], r[0], vfma<V>(wf[b], r[1], acc[24 + b]));
      acc[27] += rho;
    }
  }
  __device__ static __forceinline__ void item(const T (&x)[5], const Params& P, bool valid, T (&acc)[28]) {
    const bool v1[1] = {valid};
    item<T>(x, P, v1, acc);
  }
};

// Element offset of field f (the problem's numbering) of item i, whose offset in the streamed region is `off`: the
// problems that read S (kSPlanes) find fields 6 … 14 in the S region of the flat NDT layout.
template <typename Problem>
__device__ __forceinline__ uint64_t field_offset(const TiledLayout& L, uint64_t i, uint64_t off, int f) {
  if constexpr (Problem::kSPlanes)
    if (f >= 6) return plane_offset(L, i, ndt_stored_plane(f));
  return off + uint64_t(f) * L.field_stride;
}

}  // namespace nos
