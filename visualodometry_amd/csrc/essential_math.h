// Scalar math of the essential-matrix kernels (essential.hip): the five-point minimal solver,
// the Sampson error, the decomposition of E and the cheirality test of recoverPose.
// Host-and-device (VO_HD) so essential_host_check.cpp runs the very same code on the CPU
// against tests/essential_ref.py.  Only + - * / sqrt in fp64 and comparisons, compiled without
// FMA contraction: the host build, the device and the numpy restatement follow one operation
// order and agree to the bit (the two SVDs are pnp_math.h's jacobi_rows).
//
// The solver (Nister's formulation):
//   1. the 4-dimensional null space X, Y, Z, W of the 5 x 9 epipolar system, as the last four
//      columns of Q of a Householder QR of its transpose (no pivoting: static indices);
//   2. det E = 0 and the nine entries of E E^T E - 1/2 tr(E E^T) E = 0 for E = xX + yY + zZ + W:
//      a 10 x 20 matrix over the monomials
//        x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1;
//   3. Gaussian elimination with partial pivoting (forward on all rows, backward on rows 4..9);
//   4. rows (4,5), (6,7), (8,9) combine to a 3 x 3 matrix B(z) with B (x, y, 1)^T = 0, whose
//      determinant is a polynomial of degree 10 in z;
//   5. its real roots, ascending: the roots of each derivative bracket those of the one below,
//      and every bracket is bisected a fixed number of times (no data-dependent loop bound);
//   6. x, y from the cofactors of B at each root; (x, y, z) polished by at most three guarded
//      Gauss-Newton steps on the ten constraints themselves; E scaled to unit Frobenius norm.
// The models of a subset come out in ascending order of the root z (as found, before the
// polish): "the first model with the most inliers" of the RANSAC replay refers to this order.
#pragma once

#include "pnp_math.h"

#pragma clang fp contract(off)

namespace vo {
namespace essm {

using pnpm::Col;
using pnpm::desc_rank;
using pnpm::jacobi_rows;
using std::fabs;
using std::sqrt;

constexpr int kPts = 5;          // correspondences of the minimal solver
constexpr int kMaxModels = 10;   // real roots of the degree-10 polynomial
constexpr int kElimDoubles = 200;  // the 10 x 20 elimination matrix
constexpr int kBisect = 64;      // halvings of every root bracket
constexpr double kDblMax = 1.7976931348623157e308;

VO_HD bool finite_d(double v) { return fabs(v) <= kDblMax; }  // false for NaN and infinities

// ---------------------------------------------------------------- polynomial bookkeeping
// Variables 0: x, 1: y, 2: z, 3: 1.  Quadratic monomials by variable pair (a <= b):
// xx xy xz x yy yz y zz z 1.
__host__ __device__ constexpr int quad_idx(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo == 0 ? hi : lo == 1 ? 3 + hi : lo == 2 ? 5 + hi : 9;
}
__host__ __device__ constexpr int quad_a(int q) { return q < 4 ? 0 : q < 7 ? 1 : q < 9 ? 2 : 3; }
__host__ __device__ constexpr int quad_b(int q) { return q < 4 ? q : q < 7 ? q - 3 : q < 9 ? q - 5 : 3; }
// Column of the cubic monomial with the variables a, b, c in the elimination order above.
__host__ __device__ constexpr int cubic_col(int a, int b, int c) {
  const int ex = (a == 0) + (b == 0) + (c == 0), ey = (a == 1) + (b == 1) + (c == 1),
            ez = (a == 2) + (b == 2) + (c == 2);
  switch (ex * 16 + ey * 4 + ez) {
    case 48: return 0;   // x^3
    case 12: return 1;   // y^3
    case 36: return 2;   // x^2 y
    case 24: return 3;   // x y^2
    case 33: return 4;   // x^2 z
    case 32: return 5;   // x^2
    case 9: return 6;    // y^2 z
    case 8: return 7;    // y^2
    case 21: return 8;   // x y z
    case 20: return 9;   // x y
    case 18: return 10;  // x z^2
    case 17: return 11;  // x z
    case 16: return 12;  // x
    case 6: return 13;   // y z^2
    case 5: return 14;   // y z
    case 4: return 15;   // y
    case 3: return 16;   // z^3
    case 2: return 17;   // z^2
    case 1: return 18;   // z
    default: return 19;  // 1
  }
}

// q (+/-)= a * b for linear a, b: the 16 products in the order (i, j), each added as it is made.
template <bool NEG>
VO_HD void lin_mac(const double* a, const double* b, double (&q)[10]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double p = a[i] * b[j];
      q[quad_idx(i, j)] = NEG ? q[quad_idx(i, j)] - p : q[quad_idx(i, j)] + p;
    }
}

// c (+/-)= q * l for quadratic q and linear l: the 40 products in the order (i, j).
template <bool NEG>
VO_HD void cubic_mac(const double (&q)[10], const double* l, double (&c)[20]) {
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double p = q[i] * l[j];
      const int col = cubic_col(quad_a(i), quad_b(i), j);
      c[col] = NEG ? c[col] - p : c[col] + p;
    }
}

template <int N>
VO_HD void zero(double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
}

// ---------------------------------------------------------------- null space
// q1, q2: the five normalised correspondences.  basis[c][3 i + j]: entry (i, j) of the c-th
// null vector (X, Y, Z, W) of the rows (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1).
VO_HD void null_space5(const double (&q1)[kPts][2], const double (&q2)[kPts][2], double (&basis)[4][9]) {
  double A[9][kPts], beta[kPts];
#pragma unroll
  for (int p = 0; p < kPts; ++p) {
    const double x1 = q1[p][0], y1 = q1[p][1], x2 = q2[p][0], y2 = q2[p][1];
    A[0][p] = x2 * x1;
    A[1][p] = x2 * y1;
    A[2][p] = x2;
    A[3][p] = y2 * x1;
    A[4][p] = y2 * y1;
    A[5][p] = y2;
    A[6][p] = x1;
    A[7][p] = y1;
    A[8][p] = 1.0;
  }
#pragma unroll
  for (int k = 0; k < kPts; ++k) {
    double s2 = 0.0;
#pragma unroll
    for (int i = k; i < 9; ++i) s2 = s2 + A[i][k] * A[i][k];
    const double nrm = sqrt(s2);
    const double alpha = A[k][k] > 0 ? -nrm : nrm;
    A[k][k] = A[k][k] - alpha;  // the Householder vector stays in column k, rows k..8
    double vn = 0.0;
#pragma unroll
    for (int i = k; i < 9; ++i) vn = vn + A[i][k] * A[i][k];
    beta[k] = 2.0 / vn;
#pragma unroll
    for (int j = k + 1; j < kPts; ++j) {
      double s = 0.0;
#pragma unroll
      for (int i = k; i < 9; ++i) s = s + A[i][k] * A[i][j];
      s = s * beta[k];
#pragma unroll
      for (int i = k; i < 9; ++i) A[i][j] = A[i][j] - s * A[i][k];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = i == 5 + c ? 1.0 : 0.0;
#pragma unroll
    for (int k = kPts - 1; k >= 0; --k) {
      double s = 0.0;
#pragma unroll
      for (int i = k; i < 9; ++i) s = s + A[i][k] * v[i];
      s = s * beta[k];
#pragma unroll
      for (int i = k; i < 9; ++i) v[i] = v[i] - s * A[i][k];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) basis[c][i] = v[i];
  }
}

// ---------------------------------------------------------------- constraints
// The 10 x 20 matrix M[r * 20 + col]: row 0 det E, rows 1 + 3 i + j entry (i, j) of
// (E E^T - 1/2 tr(E E^T) I) E.
VO_HD void build_constraints(const double (&basis)[4][9], const Col& M) {
  double E[9][4];  // entry e as a linear polynomial in (x, y, z, 1)
#pragma unroll
  for (int e = 0; e < 9; ++e)
#pragma unroll
    for (int c = 0; c < 4; ++c) E[e][c] = basis[c][e];
  {
    double qa[10], qb[10], qc[10], row[20];
    zero(qa);
    zero(qb);
    zero(qc);
    zero(row);
    lin_mac<false>(E[4], E[8], qa);
    lin_mac<true>(E[5], E[7], qa);
    lin_mac<false>(E[3], E[8], qb);
    lin_mac<true>(E[5], E[6], qb);
    lin_mac<false>(E[3], E[7], qc);
    lin_mac<true>(E[4], E[6], qc);
    cubic_mac<false>(qa, E[0], row);
    cubic_mac<true>(qb, E[1], row);
    cubic_mac<false>(qc, E[2], row);
#pragma unroll
    for (int k = 0; k < 20; ++k) M[k] = row[k];
  }
  double L[6][10];  // E E^T, upper triangle: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        zero(L[e]);
#pragma unroll
        for (int k = 0; k < 3; ++k) lin_mac<false>(E[3 * i + k], E[3 * j + k], L[e]);
        ++e;
      }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      const double h = ((L[0][k] + L[3][k]) + L[5][k]) * 0.5;
      L[0][k] = L[0][k] - h;
      L[3][k] = L[3][k] - h;
      L[5][k] = L[5][k] - h;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double row[20];
      zero(row);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int lo = i < k ? i : k, hi = i < k ? k : i;
        const int e = lo == 0 ? hi : lo == 1 ? 2 + hi : 5;
        cubic_mac<false>(L[e], E[3 * k + j], row);
      }
#pragma unroll
      for (int k = 0; k < 20; ++k) M[(1 + 3 * i + j) * 20 + k] = row[k];
    }
}

// Forward elimination with partial pivoting (the first largest magnitude of the column), pivot
// rows scaled to a leading 1; then columns 5..9 cleared from the rows 4..9 above them.  False
// on a zero pivot.
VO_HD bool eliminate(const Col& M) {
  bool ok = true;
#pragma unroll 1
  for (int k = 0; k < 10; ++k) {
    int p = k;
    double big = fabs(M[k * 20 + k]);
#pragma unroll 1
    for (int r = k + 1; r < 10; ++r) {
      const double v = fabs(M[r * 20 + k]);
      if (v > big) {
        big = v;
        p = r;
      }
    }
    if (p != k) {
#pragma unroll 1
      for (int j = k; j < 20; ++j) {
        const double a = M[k * 20 + j], b = M[p * 20 + j];
        M[k * 20 + j] = b;
        M[p * 20 + j] = a;
      }
    }
    const double piv = M[k * 20 + k];
    if (piv == 0.0 || !finite_d(piv)) ok = false;
    const double inv = 1.0 / piv;
#pragma unroll 1
    for (int j = k; j < 20; ++j) M[k * 20 + j] = M[k * 20 + j] * inv;
#pragma unroll 1
    for (int r = k + 1; r < 10; ++r) {
      const double f = M[r * 20 + k];
#pragma unroll 1
      for (int j = k; j < 20; ++j) M[r * 20 + j] = M[r * 20 + j] - f * M[k * 20 + j];
    }
  }
#pragma unroll 1
  for (int k = 9; k >= 5; --k)
#pragma unroll 1
    for (int r = 4; r < k; ++r) {
      const double f = M[r * 20 + k];
#pragma unroll 1
      for (int j = k; j < 20; ++j) M[r * 20 + j] = M[r * 20 + j] - f * M[k * 20 + j];
    }
  return ok;
}

// out (+/-)= a * b, polynomials with the lowest power first; products in the order (i, j).
template <int NA, int NB, bool NEG>
VO_HD void poly_mac(const double (&a)[NA], const double (&b)[NB], double (&out)[NA + NB - 1]) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double p = a[i] * b[j];
      out[i + j] = NEG ? out[i + j] - p : out[i + j] + p;
    }
}

template <int N>
VO_HD double horner(const double (&c)[N], double z) {
  double v = c[N - 1];
#pragma unroll
  for (int k = N - 2; k >= 0; --k) v = v * z + c[k];
  return v;
}

// Rows (e, f) of the eliminated matrix: e - z f as x bx(z) + y by(z) + bc(z).
VO_HD void b_row(const Col& M, int e, int f, double (&bx)[4], double (&by)[4], double (&bc)[5]) {
  const int re = e * 20, rf = f * 20;
  bx[0] = M[re + 12];
  bx[1] = M[re + 11] - M[rf + 12];
  bx[2] = M[re + 10] - M[rf + 11];
  bx[3] = -M[rf + 10];
  by[0] = M[re + 15];
  by[1] = M[re + 14] - M[rf + 15];
  by[2] = M[re + 13] - M[rf + 14];
  by[3] = -M[rf + 13];
  bc[0] = M[re + 19];
  bc[1] = M[re + 18] - M[rf + 19];
  bc[2] = M[re + 17] - M[rf + 18];
  bc[3] = M[re + 16] - M[rf + 17];
  bc[4] = -M[rf + 16];
}

// (n + m)! / n!: coefficient n of the m-th derivative is c[n + m] times this (exact in double).
__host__ __device__ constexpr double deriv_factor(int n, int m) {
  double f = 1.0;
  for (int k = 1; k <= m; ++k) f = f * (double)(n + k);
  return f;
}

// One bracket [lo, hi] of the degree-D polynomial d: if the signs at its ends differ, kBisect
// halvings; the root goes to slot `cnt` of out.
template <int D>
VO_HD void bracket_root(const double (&d)[D + 1], double lo, double hi, double flo, double fhi,
                        double (&out)[kMaxModels], int& cnt) {
  const bool slo = flo > 0, shi = fhi > 0;
  if (slo == shi) return;
#pragma unroll 1
  for (int it = 0; it < kBisect; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool sm = horner<D + 1>(d, mid) > 0;
    lo = sm == slo ? mid : lo;
    hi = sm == slo ? hi : mid;
  }
  const double root = 0.5 * (lo + hi);
#pragma unroll
  for (int s = 0; s < kMaxModels; ++s) out[s] = s == cnt ? root : out[s];
  ++cnt;
}

// Roots of the (10 - D)-th derivative of c from those of the derivative above it (prev, padded
// with the bound B): the brackets are [-B, prev0], [prev0, prev1], ..., [prev(D-2), B].
template <int D>
VO_HD int level_roots(const double (&c)[11], double B, const double (&prev)[kMaxModels], double (&out)[kMaxModels]) {
  double d[D + 1];
#pragma unroll
  for (int i = 0; i <= D; ++i) d[i] = c[i + 10 - D] * deriv_factor(i, 10 - D);
#pragma unroll
  for (int s = 0; s < kMaxModels; ++s) out[s] = B;
  int cnt = 0;
  double lo = -B, flo = horner<D + 1>(d, lo);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const double hi = i == D - 1 ? B : prev[i];
    const double fhi = horner<D + 1>(d, hi);
    bracket_root<D>(d, lo, hi, flo, fhi, out, cnt);
    lo = hi;
    flo = fhi;
  }
  return cnt;
}

// Real roots of c (degree 10, lowest power first), ascending, inside the Cauchy bound
// 1 + max |c_i / c_10|.  0 when the leading coefficient vanishes or a coefficient is not finite.
VO_HD int real_roots10(const double (&c)[11], double (&roots)[kMaxModels]) {
  bool ok = c[10] != 0.0;
  double B = 0.0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const double r = fabs(c[i] / c[10]);
    ok = ok && finite_d(r);
    B = r > B ? r : B;
  }
  B = B + 1.0;
#pragma unroll
  for (int s = 0; s < kMaxModels; ++s) roots[s] = B;
  if (!ok) return 0;
  double a[kMaxModels], b[kMaxModels];
  level_roots<1>(c, B, roots, a);
  level_roots<2>(c, B, a, b);
  level_roots<3>(c, B, b, a);
  level_roots<4>(c, B, a, b);
  level_roots<5>(c, B, b, a);
  level_roots<6>(c, B, a, b);
  level_roots<7>(c, B, b, a);
  level_roots<8>(c, B, a, b);
  level_roots<9>(c, B, b, a);
  return level_roots<10>(c, B, a, roots);
}

// ---------------------------------------------------------------- polish
// C = A B (kind 0), A^T B (kind 1) or A B^T (kind 2) of row-major 3 x 3 matrices, each entry
// summed left to right.
template <int KIND>
VO_HD void mat3_mul(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double a = KIND == 1 ? A[3 * k + i] : A[3 * i + k];
        const double b = KIND == 2 ? B[3 * j + k] : B[3 * k + j];
        s = s + a * b;
      }
      C[3 * i + j] = s;
    }
}

// g[0] = det E, g[1 + k] = entry k of 2 E E^T E - tr(E E^T) E; also E E^T and its trace.
VO_HD void constraint_values(const double (&E)[9], double (&g)[10], double (&EEt)[9], double& tr) {
  double T[9];
  mat3_mul<2>(E, E, EEt);
  mat3_mul<0>(EEt, E, T);
  tr = (EEt[0] + EEt[4]) + EEt[8];
  g[0] = (E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6])) + E[2] * (E[3] * E[7] - E[4] * E[6]);
#pragma unroll
  for (int k = 0; k < 9; ++k) g[1 + k] = 2.0 * T[k] - tr * E[k];
}

VO_HD double sum_sq10(const double (&g)[10]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 10; ++k) s = s + g[k] * g[k];
  return s;
}

VO_HD void combine(const double (&basis)[4][9], double x, double y, double z, double (&E)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = ((x * basis[0][k] + y * basis[1][k]) + z * basis[2][k]) + basis[3][k];
}

// Up to kPolish Gauss-Newton steps of (x, y, z) on the ten constraints evaluated from
// E = xX + yY + zZ + W itself (not from the expanded polynomial, whose degree-10 root carries the
// error of the elimination): a step is kept only if it lowers the sum of squares, so a solution
// the elimination found exactly stays where it is.  The model stays in the null space.
constexpr int kPolish = 3;
VO_HD void polish(const double (&basis)[4][9], double& x, double& y, double& z) {
#pragma unroll 1
  for (int it = 0; it < kPolish; ++it) {
    double E[9], g[10], EEt[9], tr;
    combine(basis, x, y, z, E);
    constraint_values(E, g, EEt, tr);
    const double cost = sum_sq10(g);
    double EtE[9], cof[9];
    mat3_mul<1>(E, E, EtE);
    cof[0] = E[4] * E[8] - E[5] * E[7];
    cof[1] = E[5] * E[6] - E[3] * E[8];
    cof[2] = E[3] * E[7] - E[4] * E[6];
    cof[3] = E[2] * E[7] - E[1] * E[8];
    cof[4] = E[0] * E[8] - E[2] * E[6];
    cof[5] = E[1] * E[6] - E[0] * E[7];
    cof[6] = E[1] * E[5] - E[2] * E[4];
    cof[7] = E[2] * E[3] - E[0] * E[5];
    cof[8] = E[0] * E[4] - E[1] * E[3];
    double J[3][10];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double D[9], P1[9], Q[9], P2[9], P3[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) D[k] = basis[d][k];
      mat3_mul<0>(D, EtE, P1);
      mat3_mul<1>(D, E, Q);
      mat3_mul<0>(E, Q, P2);
      mat3_mul<0>(EEt, D, P3);
      double trd = 0.0, dd = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        trd = trd + E[k] * D[k];
        dd = dd + cof[k] * D[k];
      }
      J[d][0] = dd;
#pragma unroll
      for (int k = 0; k < 9; ++k) J[d][1 + k] = (2.0 * ((P1[k] + P2[k]) + P3[k]) - (2.0 * trd) * E[k]) - tr * D[k];
    }
    double a00 = 0.0, a10 = 0.0, a11 = 0.0, a20 = 0.0, a21 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      a00 = a00 + J[0][k] * J[0][k];
      a10 = a10 + J[1][k] * J[0][k];
      a11 = a11 + J[1][k] * J[1][k];
      a20 = a20 + J[2][k] * J[0][k];
      a21 = a21 + J[2][k] * J[1][k];
      a22 = a22 + J[2][k] * J[2][k];
      b0 = b0 - J[0][k] * g[k];
      b1 = b1 - J[1][k] * g[k];
      b2 = b2 - J[2][k] * g[k];
    }
    const double l10 = a10 / a00, l20 = a20 / a00;
    const double c11 = a11 - l10 * a10, c21 = a21 - l20 * a10, c22 = a22 - l20 * a20;
    const double e1 = b1 - l10 * b0, e2 = b2 - l20 * b0;
    const double l21 = c21 / c11;
    const double d2 = (e2 - l21 * e1) / (c22 - l21 * c21);
    const double d1 = (e1 - c21 * d2) / c11;
    const double d0 = ((b0 - a10 * d1) - a20 * d2) / a00;
    const double nx = x + d0, ny = y + d1, nz = z + d2;
    combine(basis, nx, ny, nz, E);
    constraint_values(E, g, EEt, tr);
    const bool take = sum_sq10(g) < cost;  // false for a step that is not finite
    x = take ? nx : x;
    y = take ? ny : y;
    z = take ? nz : z;
  }
}

// ---------------------------------------------------------------- the minimal solver
// Models of five normalised correspondences, ascending in z, unit Frobenius norm, written to
// models[9 m + e]; M is the caller's 200 doubles of work space.  Returns their number.
VO_HD int five_point(const double (&q1)[kPts][2], const double (&q2)[kPts][2], const Col& M, double* models) {
  double basis[4][9];
  null_space5(q1, q2, basis);
  build_constraints(basis, M);
  if (!eliminate(M)) return 0;
  double p1[8], p2[8], p3[7], c[11];
  {
    double bx0[4], by0[4], bc0[5], bx1[4], by1[4], bc1[5], bx2[4], by2[4], bc2[5];
    b_row(M, 4, 5, bx0, by0, bc0);
    b_row(M, 6, 7, bx1, by1, bc1);
    b_row(M, 8, 9, bx2, by2, bc2);
    zero(p1);
    zero(p2);
    zero(p3);
    zero(c);
    poly_mac<4, 5, false>(by1, bc2, p1);
    poly_mac<5, 4, true>(bc1, by2, p1);
    poly_mac<4, 5, false>(bx1, bc2, p2);
    poly_mac<5, 4, true>(bc1, bx2, p2);
    poly_mac<4, 4, false>(bx1, by2, p3);
    poly_mac<4, 4, true>(by1, bx2, p3);
    poly_mac<4, 8, false>(bx0, p1, c);
    poly_mac<4, 8, true>(by0, p2, c);
    poly_mac<5, 7, false>(bc0, p3, c);
  }
  double roots[kMaxModels];
  const int nr = real_roots10(c, roots);
  int nm = 0;
#pragma unroll 1
  for (int r = 0; r < nr; ++r) {
    double z = roots[0];
#pragma unroll
    for (int s = 1; s < kMaxModels; ++s) z = s == r ? roots[s] : z;
    const double den = horner<7>(p3, z);
    double x = horner<8>(p1, z) / den;
    double y = -horner<8>(p2, z) / den;
    polish(basis, x, y, z);
    double e[9], n2 = 0.0;
    combine(basis, x, y, z, e);
#pragma unroll
    for (int k = 0; k < 9; ++k) n2 = n2 + e[k] * e[k];
    const double inv = 1.0 / sqrt(n2);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      e[k] = e[k] * inv;
      fin = fin && finite_d(e[k]);
    }
    if (!fin) continue;
#pragma unroll
    for (int k = 0; k < 9; ++k) models[9 * nm + k] = e[k];
    ++nm;
  }
  return nm;
}

// ---------------------------------------------------------------- scoring
// Pixel to normalised coordinates, in double.
VO_HD void normalise(float u, float v, const pnpm::Cam& K, double& x, double& y) {
  x = ((double)u - K.uc) / K.fu;
  y = ((double)v - K.vc) / K.fv;
}

// Sampson error of (x1, y1) <-> (x2, y2) under E (row-major), double, cast to float32.
VO_HD float sampson_f32(const double* E, double x1, double y1, double x2, double y2) {
  const double a0 = (E[0] * x1 + E[1] * y1) + E[2];
  const double a1 = (E[3] * x1 + E[4] * y1) + E[5];
  const double a2 = (E[6] * x1 + E[7] * y1) + E[8];
  const double b0 = (E[0] * x2 + E[3] * y2) + E[6];
  const double b1 = (E[1] * x2 + E[4] * y2) + E[7];
  const double d = (x2 * a0 + y2 * a1) + a2;
  return (float)(d * d / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1));
}

// (float)(thr_n^2) with thr_n = threshold / ((fx + fy) / 2): a point is an inlier at err <= this.
VO_HD float sampson_threshold(double threshold, const pnpm::Cam& K) {
  const double tn = threshold / ((K.fu + K.fv) / 2.0);
  return (float)(tn * tn);
}

// ---------------------------------------------------------------- RANSAC replay
// The serial loop of RANSACPointSetRegistrator::run over precomputed inlier counts, with several
// models per iteration: models are visited in (iteration, model) order, a model becomes the best
// when its count is > max(best, 4), niters is updated at once and bounds the iterations only.
struct Replay {
  int it, niters, best_it, best_m, max_good;
};
VO_HD Replay replay_start(int max_iters) { return Replay{0, max_iters, -1, 0, 0}; }
// Iterations [r.it, stop) with nmodels[it - base] models each and counts[(it - base) * 10 + m].
VO_HD void replay_range(Replay& r, const int* nmodels, const int* counts, int base, int stop, int n, double prob) {
  for (; r.it < r.niters && r.it < stop; ++r.it) {
    const int nm = nmodels[r.it - base];
    for (int m = 0; m < nm; ++m) {
      const int good = counts[(r.it - base) * kMaxModels + m];
      if (good > (r.max_good > kPts - 1 ? r.max_good : kPts - 1)) {
        r.best_it = r.it;
        r.best_m = m;
        r.max_good = good;
        r.niters = pnpm::update_num_iters(prob, (double)(n - good) / n, kPts, r.niters);
      }
    }
  }
}

// ---------------------------------------------------------------- recoverPose
// E = U diag(s, s, 0) V^T by jacobi_rows on the rows of E^T.  The third left vector, which the
// one-sided Jacobi leaves undefined at a zero singular value, is the cross product of the first
// two (so det U = +1); V^T is negated when its determinant is negative.  R1 = U W V^T,
// R2 = U W^T V^T with W = [[0,1,0],[-1,0,0],[0,0,1]], t = the third column of U.
VO_HD void decompose_essential(const double* E, double (&R1)[9], double (&R2)[9], double (&t)[3]) {
  double At[3][3], Wv[3], Vt[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) At[a][b] = E[3 * b + a];
  jacobi_rows<3, 3, true>(At, Wv, Vt);
  int rk[3];
  desc_rank<3>(Wv, rk);
  double u[3][3], v[3][3];  // u[q]: the q-th left vector, v[q]: the q-th row of V^T
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u[q][k] = 0.0;
      v[q][k] = 0.0;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double iw = 1.0 / Wv[i];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        u[q][k] = rk[i] == q ? At[i][k] * iw : u[q][k];
        v[q][k] = rk[i] == q ? Vt[i][k] : v[q][k];
      }
  }
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  const double det = (v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) -
                      v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0])) +
                     v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
  if (det < 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int k = 0; k < 3; ++k) v[q][k] = -v[q][k];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R1[3 * i + j] = (-u[1][i] * v[0][j] + u[0][i] * v[1][j]) + u[2][i] * v[2][j];
      R2[3 * i + j] = (u[1][i] * v[0][j] - u[0][i] * v[1][j]) + u[2][i] * v[2][j];
    }
    t[i] = u[2][i];
  }
}

// One correspondence under the candidate [R | t] against [I | 0]: the DLT point (right singular
// vector of the smallest singular value of the 4 x 4 system), then recoverPose's tests.
VO_HD bool cheirality(const double* R, const double* t, double x1, double y1, double x2, double y2, double dist) {
  double At[4][4], Wv[4], Vt[4][4];  // At: the transpose of the DLT rows
  At[0][0] = -1.0;
  At[1][0] = 0.0;
  At[2][0] = x1;
  At[3][0] = 0.0;
  At[0][1] = 0.0;
  At[1][1] = -1.0;
  At[2][1] = y1;
  At[3][1] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    At[k][2] = x2 * R[6 + k] - R[k];
    At[k][3] = y2 * R[6 + k] - R[3 + k];
  }
  At[3][2] = x2 * t[2] - t[0];
  At[3][3] = y2 * t[2] - t[1];
  jacobi_rows<4, 4, true>(At, Wv, Vt);
  int rk[4];
  desc_rank<4>(Wv, rk);
  double Q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) Q[k] = rk[i] == 3 ? Vt[i][k] : Q[k];
  bool ok = Q[2] * Q[3] > 0;
  const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3];
  ok = ok && Z < dist;
  const double z2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
  ok = ok && z2 > 0 && z2 < dist;
  return ok;
}

}  // namespace essm
}  // namespace vo
