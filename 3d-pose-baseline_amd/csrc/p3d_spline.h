// p3d_spline.h -- the reference's --interpolation stage (src/openpose_3dpose_sandbox.py:240-291) on
// the device: every one of a clip's 36 smoothed tracks is fitted with scipy's
// UnivariateSpline(frame, y, k=3) followed by set_smoothing_factor((max - min) * 125), that is
// FITPACK's fpcurf for k = 3, unit weights and the abscissae 0 .. m - 1 run twice, the second run
// (iopt = 1) continuing from the knots, fpint and nrdata of the first; the spline is then sampled at
// j * (1 / R) by splev's arithmetic and the samples become the model's input rows.
//
//   k_spline_fit    one wave per curve (clip, column): stage 1, S, stage 2 -> t, c, info
//   k_spline_rows   64 output rows per workgroup: splev, xy_r, the x rows (clip_x_value), off_out
//
// All of it is float64 with contraction off and uses + - * /, sqrt and fabs only, in the order of
// tests/spline_oracle.py, so coefficients and samples carry the oracle's bits.  A curve's Givens
// sweeps are one serial recurrence whose order is part of the result: lane 0 runs the fit, the
// wave's lanes stage the track and copy the result.  The curve's state lives in LDS while
// SPL_STATE(m) doubles fit the launch's dynamic LDS and in the curve's own slice of the workspace
// beyond that.  No workgroup waits for another, there are no atomics and nothing depends on the
// grid: the rows kernel strides over a clip's chunks, the fit kernel over the curves.
//
// Arrays are addressed 1-based as in the Fortran text (pointer - 1), so the indices read as FITPACK's.
#pragma once
#include "p3d_clips.h"

#define P3D_SPL_MAX_R 16
#define P3D_SPL_MIN_M 4            // FITPACK: m > k
#define P3D_SPL_MAX_M 65536
#define P3D_SPL_ROWS 64            // output rows per workgroup of k_spline_rows
#define P3D_SPL_LDS_BYTES 65536    // the fit's dynamic LDS at most
#define P3D_SPL_INFO 5             // n after stage 1, n after stage 2, ier of stage 1, of stage 2, p iterations
#define P3D_SPL_IER_NO_INTERVAL 5  // ours: no knot interval can take a knot (FITPACK reads an unset index there)

// doubles of state per curve of m frames: t c z fpint [nest] | a [nest, 4] | g b [nest, 5] | q [m, 4] |
// y [m] | nrdata i32 [nest], nest = m + 4
#define SPL_STATE(m) (24 * ((int64_t)(m) + 4))
// where curve (clip at rows lo.., number s; column col) keeps its nest = m + 4 knots / coefficients
#define SPL_COEF_AT(lo, s, col, m) (36 * ((int64_t)(lo) + 4 * (int64_t)(s)) + (int64_t)(col) * ((int64_t)(m) + 4))

#if defined(__HIPCC__)
#define P3D_SPL_HD __host__ __device__ __forceinline__
#else
#define P3D_SPL_HD inline
#endif

struct SplState {
  double *t, *c, *z, *fpint, *a, *g, *b, *q;   // 1-based
  int32_t* nrdata;                             // 1-based
  int n, ier, iters;
  double fp;
};

P3D_SPL_HD void spl_carve(SplState& st, double* base, int m) {
  const int nest = m + 4;
  double* p = base;
  st.t = p - 1; p += nest;
  st.c = p - 1; p += nest;
  st.z = p - 1; p += nest;
  st.fpint = p - 1; p += nest;
  st.a = p; p += 4 * nest;
  st.g = p; p += 5 * nest;
  st.b = p; p += 5 * nest;
  st.q = p; p += 4 * m;
  p += m;                                       // y (spl_y)
  st.nrdata = reinterpret_cast<int32_t*>(p) - 1;
  st.n = 0; st.ier = 0; st.iters = 0; st.fp = 0.0;
}
P3D_SPL_HD double* spl_y(double* base, int m) { return base + 18 * (m + 4) + 4 * m - 1; }   // 1-based

#define SPL_A(i, j) st.a[((i) - 1) * 4 + (j) - 1]
#define SPL_G(i, j) st.g[((i) - 1) * 5 + (j) - 1]
#define SPL_B(i, j) st.b[((i) - 1) * 5 + (j) - 1]
#define SPL_Q(i, j) st.q[((i) - 1) * 4 + (j) - 1]

// the four cubic B-splines that are non-zero on t[l] <= x < t[l + 1] -> h[1..4] (fpbspl)
P3D_SPL_HD void spl_bspl(const double* t, double x, int l, double* h) {
#pragma clang fp contract(off)
  double hh[6];
  h[1] = 1.0;
  for (int j = 1; j <= 3; ++j) {
    for (int i = 1; i <= j; ++i) hh[i] = h[i];
    h[1] = 0.0;
    for (int i = 1; i <= j; ++i) {
      const int li = l + i, lj = li - j;
      const double tli = t[li], tlj = t[lj];
      if (tli == tlj) { h[i + 1] = 0.0; continue; }
      const double f = hh[i] / (tli - tlj);
      h[i] = h[i] + f * (tli - x);
      h[i + 1] = f * (x - tlj);
    }
  }
}

P3D_SPL_HD void spl_givs(double piv, double& ww, double& cs, double& sn) {   // fpgivs
#pragma clang fp contract(off)
  const double store = fabs(piv);
  double dd;
  if (store >= ww) { const double r = ww / piv; dd = store * sqrt(1.0 + r * r); }
  else { const double r = piv / ww; dd = ww * sqrt(1.0 + r * r); }
  cs = ww / dd;
  sn = piv / dd;
  ww = dd;
}

P3D_SPL_HD void spl_rota(double cs, double sn, double& a, double& b) {       // fprota
#pragma clang fp contract(off)
  const double s1 = a, s2 = b;
  b = cs * s2 + sn * s1;
  a = cs * s1 - sn * s2;
}

// fpback: a [n, w] the triangle's rows (band k), z the right-hand side, c the solution (c may be z)
P3D_SPL_HD void spl_back(const double* a, int w, const double* z, int n, int k, double* c) {
#pragma clang fp contract(off)
  const int k1 = k - 1;
  c[n] = z[n] / a[(n - 1) * w];
  int i = n - 1;
  for (int j = 2; j <= n; ++j) {
    double store = z[i];
    const int i1 = j <= k1 ? j - 1 : k1;
    int mm = i;
    for (int l = 1; l <= i1; ++l) {
      ++mm;
      store = store - c[mm] * a[(i - 1) * w + l];
    }
    c[i] = store / a[(i - 1) * w];
    --i;
  }
}

P3D_SPL_HD void spl_disc(SplState& st, int n) {                              // fpdisc, k2 = 5
#pragma clang fp contract(off)
  const double* t = st.t;
  const int nk1 = n - 4, nrint = nk1 - 3;
  const double fac = (double)nrint / (t[nk1 + 1] - t[4]);
  double h[13];
  for (int l = 5; l <= nk1; ++l) {
    const int lmk = l - 4;
    for (int j = 1; j <= 4; ++j) {
      const int ik = j + 4, lj = l + j, lk = lj - 5;
      h[j] = t[l] - t[lk];
      h[ik] = t[l] - t[lj];
    }
    int lp = lmk;
    for (int j = 1; j <= 5; ++j) {
      int jk = j;
      double prod = h[j];
      for (int i = 1; i <= 3; ++i) {
        ++jk;
        prod = prod * h[jk] * fac;
      }
      const int lk = lp + 4;
      SPL_B(lmk, j) = (t[lk] - t[lp]) / prod;
      ++lp;
    }
  }
}

// fpknot: one more knot in the interval whose residual sum is largest; false: no interval can take one
P3D_SPL_HD bool spl_knot(SplState& st, int nrint) {
#pragma clang fp contract(off)
  double* t = st.t;
  double* fpint = st.fpint;
  int32_t* nrdata = st.nrdata;
  const int k = (st.n - nrint - 1) / 2;
  double fpmax = 0.0;
  int jbegin = 1, number = 0, maxpt = 0, maxbeg = 0;
  for (int j = 1; j <= nrint; ++j) {
    const int jpoint = nrdata[j];
    if (!(fpmax >= fpint[j]) && jpoint != 0) {
      fpmax = fpint[j];
      number = j; maxpt = jpoint; maxbeg = jbegin;
    }
    jbegin = jbegin + jpoint + 1;
  }
  if (number == 0) return false;
  const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf, nxt = number + 1;
  for (int j = nxt; j <= nrint; ++j) {
    const int jj = nxt + nrint - j;
    fpint[jj + 1] = fpint[jj];
    nrdata[jj + 1] = nrdata[jj];
    const int jk = jj + k;
    t[jk + 1] = t[jk];
  }
  nrdata[number] = ihalf - 1;
  nrdata[nxt] = maxpt - ihalf;
  const double am = (double)maxpt;
  double an = (double)nrdata[number];
  fpint[number] = fpmax * an / am;
  an = (double)nrdata[nxt];
  fpint[nxt] = fpmax * an / am;
  t[nxt + k] = (double)(nrx - 1);               // x(nrx), the abscissae being 0 .. m - 1
  st.n += 1;
  return true;
}

P3D_SPL_HD void spl_interp_knots(SplState& st, int m) {
  int i = 5, j = 3;
  for (int q = 0; q < m - 4; ++q) { st.t[i] = (double)(j - 1); ++i; ++j; }
}

// FITPACK fpcurf, k = 3, w = 1, x = 0 .. m - 1, tol = 0.001, maxit = 20.  y is 1-based.
// iopt = 1 continues from st.n, st.t, st.fpint and st.nrdata as the call before left them.  nest: the
// knots the caller has room for (scipy: max(m / 2, 8) at first; ier = 1 where more are needed, and the
// call is then continued with room for all m + 4).  ier_in: what the caller's ier holds on entry --
// scipy passes the last call's on, and a non-zero one makes the first knot round add one knot.
P3D_SPL_HD void spl_fpcurf(int iopt, int m, const double* y, double s, SplState& st, int nest, int ier_in) {
#pragma clang fp contract(off)
  double* t = st.t;
  double* c = st.c;
  double* z = st.z;
  double* fpint = st.fpint;
  int32_t* nrdata = st.nrdata;
  const double xb = 0.0, xe = (double)(m - 1);
  const double acc = 0.001 * s;
  const int nmax = m + 4;
  int ier = ier_in, nplus = 0;
  double fp0 = 0.0, fpold = 0.0;
  st.iters = 0;

  bool restart = true;
  if (s > 0.0) {
    if (iopt != 0 && st.n != 8) {
      fp0 = fpint[st.n];
      fpold = fpint[st.n - 1];
      nplus = nrdata[st.n];
      restart = !(fp0 > s);
    }
    if (restart) {
      st.n = 8;
      fpold = 0.0;
      nplus = 0;
      nrdata[1] = m - 2;
    }
  } else {
    st.n = nmax;
    if (nmax > nest) { st.ier = 1; return; }
    spl_interp_knots(st, m);
  }

  double fp = 0.0, fpms = 0.0;
  int nk1 = 0;
  bool accept = false, done = false;            // the knots stand (label 250); label 440
  while (!done && !accept) {
    bool again = false;
    int round = 0;
    for (; round < m; ++round) {
      const int n = st.n;
      if (n == 8) ier = -2;
      int nrint = n - 8 + 1;
      nk1 = n - 4;
      {
        int i = n;
        for (int j = 1; j <= 4; ++j) { t[j] = xb; t[i] = xe; --i; }
      }
      fp = 0.0;
      for (int i = 1; i <= nk1; ++i) {
        z[i] = 0.0;
        SPL_A(i, 1) = 0.0; SPL_A(i, 2) = 0.0; SPL_A(i, 3) = 0.0; SPL_A(i, 4) = 0.0;
      }
      int l = 4;
      for (int it = 1; it <= m; ++it) {
        const double xi = (double)(it - 1);
        double yi = y[it];
        while (!(xi < t[l + 1] || l == nk1)) ++l;
        double h[6];
        spl_bspl(t, xi, l, h);
        SPL_Q(it, 1) = h[1]; SPL_Q(it, 2) = h[2]; SPL_Q(it, 3) = h[3]; SPL_Q(it, 4) = h[4];
        int j = l - 4;
        for (int i = 1; i <= 4; ++i) {
          ++j;
          const double piv = h[i];
          if (piv == 0.0) continue;
          double cs, sn;
          spl_givs(piv, SPL_A(j, 1), cs, sn);
          spl_rota(cs, sn, yi, z[j]);
          if (i == 4) break;
          int i2 = 1;
          for (int i1 = i + 1; i1 <= 4; ++i1) {
            ++i2;
            spl_rota(cs, sn, h[i1], SPL_A(j, i2));
          }
        }
        fp = fp + yi * yi;
      }
      if (ier == -2) fp0 = fp;
      fpint[n] = fp0;
      fpint[n - 1] = fpold;
      nrdata[n] = nplus;
      spl_back(st.a, 4, z, nk1, 4, c);
      fpms = fp - s;
      if (fabs(fpms) < acc) { done = true; break; }
      if (fpms < 0.0) { accept = true; break; }
      if (n == nmax) { ier = -1; done = true; break; }
      if (n == nest) { ier = 1; done = true; break; }
      if (ier != 0) {
        nplus = 1;
        ier = 0;
      } else {
        int npl1 = nplus * 2;
        const double rn = (double)nplus;
        if (fpold - fp > acc) {
          const double v = rn * fpms / (fpold - fp);
          npl1 = (v == v && fabs(v) < 2147483648.0) ? (int)v : (-2147483647 - 1);
        }
        int hi = npl1 > nplus / 2 ? npl1 : nplus / 2;
        if (hi < 1) hi = 1;
        nplus = nplus * 2 < hi ? nplus * 2 : hi;
      }
      fpold = fp;
      double fpart = 0.0;
      {
        int i = 1, nw = 0;
        l = 5;
        for (int it = 1; it <= m; ++it) {
          if (!((double)(it - 1) < t[l] || l > nk1)) { nw = 1; ++l; }
          double term = 0.0;
          int l0 = l - 5;
          for (int j = 1; j <= 4; ++j) {
            ++l0;
            term = term + c[l0] * SPL_Q(it, j);
          }
          term = (term - y[it]) * (term - y[it]);
          fpart = fpart + term;
          if (nw) {
            const double store = term * 0.5;
            fpint[i] = fpart - store;
            ++i;
            fpart = store;
            nw = 0;
          }
        }
      }
      fpint[nrint] = fpart;
      for (int q = 0; q < nplus; ++q) {
        if (!spl_knot(st, nrint)) { ier = P3D_SPL_IER_NO_INTERVAL; done = true; break; }
        ++nrint;
        if (st.n == nmax) { spl_interp_knots(st, m); again = true; break; }   // (go to 10, then 60)
        if (st.n == nest) break;
      }
      if (done || again) break;
    }
    if (round == m) accept = true;               // m rounds: on to label 250
    if (again) continue;
  }

  if (accept && ier != -2) {
    const int n = st.n;
    nk1 = n - 4;
    spl_disc(st, n);
    double p1 = 0.0, f1 = fp0 - s, p3 = -1.0, f3 = fpms, p = 0.0;
    for (int i = 1; i <= nk1; ++i) p = p + SPL_A(i, 1);
    p = (double)nk1 / p;
    int ich1 = 0, ich3 = 0;
    const int n8 = n - 8;
    double h[7];
    for (int itp = 1; itp <= 20; ++itp) {
      st.iters = itp;
      const double pinv = 1.0 / p;
      for (int i = 1; i <= nk1; ++i) {
        c[i] = z[i];
        SPL_G(i, 5) = 0.0;
        SPL_G(i, 1) = SPL_A(i, 1); SPL_G(i, 2) = SPL_A(i, 2); SPL_G(i, 3) = SPL_A(i, 3); SPL_G(i, 4) = SPL_A(i, 4);
      }
      for (int it = 1; it <= n8; ++it) {
        for (int i = 1; i <= 5; ++i) h[i] = SPL_B(it, i) * pinv;
        double yi = 0.0;
        for (int j = it; j <= nk1; ++j) {
          const double piv = h[1];
          double cs, sn;
          spl_givs(piv, SPL_G(j, 1), cs, sn);
          spl_rota(cs, sn, yi, c[j]);
          if (j == nk1) break;
          const int i2 = j <= n8 ? 4 : nk1 - j;
          for (int i = 1; i <= i2; ++i) {
            const int i1 = i + 1;
            spl_rota(cs, sn, h[i1], SPL_G(j, i1));
            h[i] = h[i1];
          }
          h[i2 + 1] = 0.0;
        }
      }
      spl_back(st.g, 5, c, nk1, 5, c);
      fp = 0.0;
      int l = 5;
      for (int it = 1; it <= m; ++it) {
        if (!((double)(it - 1) < t[l] || l > nk1)) ++l;
        int l0 = l - 5;
        double term = 0.0;
        for (int j = 1; j <= 4; ++j) {
          ++l0;
          term = term + c[l0] * SPL_Q(it, j);
        }
        fp = fp + (term - y[it]) * (term - y[it]);
      }
      fpms = fp - s;
      if (fabs(fpms) < acc) break;
      if (itp == 20) { ier = 3; break; }
      const double p2 = p, f2 = fpms;
      if (ich3 == 0) {
        if (!(f2 - f3 > acc)) {
          p3 = p2; f3 = f2;
          p = p * 0.04;
          if (p <= p1) p = p1 * 0.9 + p2 * 0.1;
          continue;
        }
        if (f2 < 0.0) ich3 = 1;
      }
      if (ich1 == 0) {
        if (!(f1 - f2 > acc)) {
          p1 = p2; f1 = f2;
          p = p / 0.04;
          if (p3 < 0.0) continue;
          if (p >= p3) p = p2 * 0.1 + p3 * 0.9;
          continue;
        }
        if (f2 > 0.0) ich1 = 1;
      }
      if (f2 >= f1 || f2 <= f3) { ier = 2; break; }
      // fprati
      if (p3 > 0.0) {
        const double h1 = f1 * (f2 - f3), h2 = f2 * (f3 - f1), h3 = f3 * (f1 - f2);
        p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3);
      } else {
        p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3);
      }
      if (f2 < 0.0) { p3 = p2; f3 = f2; }
      else { p1 = p2; f1 = f2; }
    }
  }
  for (int i = st.n - 3; i <= st.n; ++i) c[i] = 0.0;   // (the four unused coefficients)
  st.fp = fp;
  st.ier = ier;
}

// (max - min) * 125 as the reference forms it: Python's min / max, strict compares in position order
P3D_SPL_HD double spl_span_factor(const double* y, int m) {
#pragma clang fp contract(off)
  double lo = y[1], hi = y[1];
  for (int i = 2; i <= m; ++i) {
    const double v = y[i];
    if (v < lo) lo = v;
    if (v > hi) hi = v;
  }
  return (hi - lo) * 125.0;
}

// the reference's two calls on one track (y 1-based inside `base`'s y slot) -> st, info [5]
P3D_SPL_HD void spl_fit_curve(double* base, int m, SplState& st, int32_t* info) {
  const double* y = spl_y(base, m);
  int nest = m / 2 > 8 ? m / 2 : 8;
  spl_fpcurf(0, m, y, (double)m, st, nest, 0);
  if (st.ier == 1) {
    nest = m + 4;
    spl_fpcurf(1, m, y, (double)m, st, nest, 1);
  }
  info[0] = st.n; info[2] = st.ier;
  const double S = spl_span_factor(y, m);
  spl_fpcurf(1, m, y, S, st, nest, st.ier);
  if (st.ier == 1) spl_fpcurf(1, m, y, S, st, m + 4, 1);
  info[1] = st.n; info[3] = st.ier; info[4] = st.iters;
}

// s(arg) by splev's arithmetic (ext = 0: the end pieces extrapolate); t, c 1-based [n]
P3D_SPL_HD double spl_eval(const double* t, const double* c, int n, double arg) {
#pragma clang fp contract(off)
  const int nk1 = n - 4;
  int lo = 4, hi = nk1;                          // the largest l in [4, nk1] with t[l] <= arg (4 if none)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= arg) lo = mid; else hi = mid - 1;
  }
  double h[6];
  spl_bspl(t, arg, lo, h);
  double sp = 0.0;
  int ll = lo - 4;
  for (int j = 1; j <= 4; ++j) {
    ++ll;
    sp = sp + c[ll] * h[j];
  }
  return sp;
}

#if defined(__HIPCC__)
struct SplArgs {
  const double* xy_s;    // [N, 36] the smoothed held tracks
  int64_t N;
  int R;
  double* tcoef;         // workspace [36 (N + 4 S)]: curve (s, col) at SPL_COEF_AT
  double* ccoef;         // the same
  double* state;         // workspace [36 (N + 4 S) * 24]: the state of curves too long for LDS
  int32_t* info;         // [S, 36, 5] (workspace, or the caller's)
  int64_t lds_doubles;   // the launch's dynamic LDS
  double* xy_r;          // [R N, 36]
  int64_t* off_out;      // [S + 1]
};

__global__ __launch_bounds__(64) void k_spline_fit(SplArgs a, ClipSeg sg) {
  extern __shared__ double spl_lds[];
  __shared__ int s_n;
  const int lane = threadIdx.x;
  for (int64_t cv = blockIdx.x; cv < sg.S * P3D_CLIP_COLS; cv += gridDim.x) {
    const int64_t s = cv / P3D_CLIP_COLS;
    const int col = (int)(cv - s * P3D_CLIP_COLS);
    int64_t lo, hi;
    clip_bounds(sg, a.N, s, lo, hi);
    const int64_t mm = hi - lo;
    int32_t* info = a.info + cv * P3D_SPL_INFO;
    if (mm < P3D_SPL_MIN_M || mm > P3D_SPL_MAX_M) {   // (device offsets the host never saw: no curve)
      if (lane < P3D_SPL_INFO) info[lane] = 0;
      continue;
    }
    const int m = (int)mm;
    const int64_t at = SPL_COEF_AT(lo, s, col, m);
    double* base = SPL_STATE(m) <= a.lds_doubles ? spl_lds : a.state + at * 24;
    double* y = spl_y(base, m);
    for (int i = lane; i < m; i += 64) y[i + 1] = a.xy_s[(lo + i) * P3D_CLIP_COLS + col];
    __syncthreads();
    SplState st;
    spl_carve(st, base, m);
    if (lane == 0) {
      int32_t inf[P3D_SPL_INFO];
      spl_fit_curve(base, m, st, inf);
      for (int q = 0; q < P3D_SPL_INFO; ++q) info[q] = inf[q];
      s_n = st.n;
    }
    __syncthreads();
    const int nest = m + 4, n = s_n;
    for (int i = lane; i < nest; i += 64) {   // (the slots past n: zeros, not what the state held before)
      a.tcoef[at + i] = i < n ? st.t[i + 1] : 0.0;
      a.ccoef[at + i] = i < n ? st.c[i + 1] : 0.0;
    }
    __syncthreads();
  }
}

// blockIdx.x: the clip (strided), blockIdx.y: the clip's chunk of 64 output rows (strided)
__global__ __launch_bounds__(P3D_CLIP_THREADS) void k_spline_rows(SplArgs a, ClipInArgs in, ClipSeg sg) {
#pragma clang fp contract(off)
  constexpr int NC = P3D_CLIP_COLS, RW = P3D_SPL_ROWS;
  __shared__ double srow[RW * NC];
  __shared__ ClipMap mp;
  const int t = threadIdx.x;
  const int64_t R = a.R;
  const double step = 1.0 / (double)a.R;
  clip_load_map(in, mp);
  for (int64_t s = blockIdx.x; s < sg.S; s += gridDim.x) {
    int64_t lo, hi;
    clip_bounds(sg, a.N, s, lo, hi);
    const int64_t m = hi - lo, rows = R * m;
    if (blockIdx.y == 0 && t == 0) {
      a.off_out[s] = R * lo;
      if (s == sg.S - 1) a.off_out[sg.S] = R * hi;
    }
    const bool fitted = m >= P3D_SPL_MIN_M && m <= P3D_SPL_MAX_M;
    for (int64_t j0 = (int64_t)blockIdx.y * RW; j0 < rows; j0 += (int64_t)gridDim.y * RW) {
      __syncthreads();
      for (int idx = t; idx < RW * NC; idx += P3D_CLIP_THREADS) {
        const int col = idx / RW, i = idx - col * RW;    // a wave's lanes share the curve
        const int64_t j = j0 + i;
        double v = 0.0;
        if (j < rows && fitted) {
          const int n = a.info[(s * NC + col) * P3D_SPL_INFO + 1];
          const int64_t at = SPL_COEF_AT(lo, s, col, m);
          if (n >= 8 && n <= m + 4) v = spl_eval(a.tcoef + at - 1, a.ccoef + at - 1, n, (double)j * step);
        }
        srow[i * NC + col] = v;
      }
      __syncthreads();
      const int64_t r0 = R * lo + j0;
      for (int idx = t; idx < RW * NC; idx += P3D_CLIP_THREADS) {
        const int i = idx / NC;
        if (j0 + i < rows) a.xy_r[r0 * NC + idx] = srow[idx];
      }
      clip_write_x(in, srow, r0, RW, mp, R * hi);
    }
  }
}
#endif
