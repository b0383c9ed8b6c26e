"""The spline resampling of DESIGN.md 8f in plain float64 scalar arithmetic: FITPACK's fpcurf for
k = 3, unit weights and the abscissae 0, 1, ..., m - 1, run twice as the reference's
UnivariateSpline(frame, y, k=3) followed by set_smoothing_factor((max - min) * 125) runs it (the second
call continues from the first call's knots, fpint and nrdata), and splev's evaluation.  Every
operation is written in the order csrc/p3d_spline.h performs it, so the kernel's coefficients and
samples are compared with these as bytes.  Python floats are IEEE doubles and math.sqrt rounds
correctly; nothing here contracts a multiply and an add.

Arrays are 1-based as in the Fortran text (slot 0 unused), so the indices read as FITPACK's."""
import math

import numpy as np

TOL = 0.001
MAXIT = 20
CON1, CON9, CON4, HALF = 0.1, 0.9, 0.04, 0.5
K, K1, K2, NMIN = 3, 4, 5, 8


class Margins:
    """The smallest relative gap by which any discrete decision of a fit was taken."""

    def __init__(self):
        self.m = math.inf
        self.what = ""

    def cmp(self, a, b, what=""):
        if a != a or b != b:
            return
        d = max(abs(a), abs(b))
        if d > 0.0 and abs(a - b) / d < self.m:
            self.m, self.what = abs(a - b) / d, what

    def trunc(self, v):
        """v is about to be truncated to an integer: its distance from the nearest whole number."""
        if v == v and 1.0 <= abs(v) < 1e15:
            g = min(v - math.floor(v), math.floor(v) + 1.0 - v) / abs(v)
            if g < self.m:
                self.m, self.what = g, "npl1"



def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(v):
    if v != v or v < 0.0:
        return math.nan
    return math.sqrt(v)


def span_factor(y):
    """(max - min) * 125 with Python's min / max: strict compares in position order."""
    lo = hi = y[0]
    for v in y[1:]:
        if v < lo:
            lo = v
        if v > hi:
            hi = v
    return (hi - lo) * 125.0


def fpbspl(t, x, l):
    """The four cubic B-splines that are non-zero on t[l] <= x < t[l + 1] (h[1..4])."""
    h = [0.0] * 6
    hh = [0.0] * 6
    h[1] = 1.0
    for j in range(1, K + 1):
        for i in range(1, j + 1):
            hh[i] = h[i]
        h[1] = 0.0
        for i in range(1, j + 1):
            li = l + i
            lj = li - j
            if t[li] == t[lj]:
                h[i + 1] = 0.0
                continue
            f = _div(hh[i], t[li] - t[lj])
            h[i] = h[i] + f * (t[li] - x)
            h[i + 1] = f * (x - t[lj])
    return h


def fpgivs(piv, ww):
    store = abs(piv)
    if store >= ww:
        r = _div(ww, piv)
        dd = store * _sqrt(1.0 + r * r)
    else:
        r = _div(piv, ww)
        dd = ww * _sqrt(1.0 + r * r)
    return dd, _div(ww, dd), _div(piv, dd)      # ww, cos, sin


def fprota(cos, sin, a, b):
    return cos * a - sin * b, cos * b + sin * a  # a, b


def fpback(a, z, n, k, c):
    k1 = k - 1
    c[n] = _div(z[n], a[n][1])
    i = n - 1
    for j in range(2, n + 1):
        store = z[i]
        i1 = j - 1 if j <= k1 else k1
        mm = i
        for l in range(1, i1 + 1):
            mm += 1
            store = store - c[mm] * a[i][l + 1]
        c[i] = _div(store, a[i][1])
        i -= 1


def fpdisc(t, n, b):
    nk1 = n - K1
    nrint = nk1 - K
    fac = _div(float(nrint), t[nk1 + 1] - t[K1])
    h = [0.0] * 13
    for l in range(K2, nk1 + 1):
        lmk = l - K1
        for j in range(1, K1 + 1):
            ik = j + K1
            lj = l + j
            lk = lj - K2
            h[j] = t[l] - t[lk]
            h[ik] = t[l] - t[lj]
        lp = lmk
        for j in range(1, K2 + 1):
            jk = j
            prod = h[j]
            for _ in range(K):
                jk += 1
                prod = prod * h[jk] * fac
            lk = lp + K1
            b[lmk][j] = _div(t[lk] - t[lp], prod)
            lp += 1


def fprati(p1, f1, p2, f2, p3, f3):
    if p3 > 0.0:
        h1 = f1 * (f2 - f3)
        h2 = f2 * (f3 - f1)
        h3 = f3 * (f1 - f2)
        p = _div(-(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2), p1 * h1 + p2 * h2 + p3 * h3)
    else:
        p = _div(p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1, (f1 - f2) * f3)
    if f2 < 0.0:
        p3, f3 = p2, f2
    else:
        p1, f1 = p2, f2
    return p, p1, f1, p3, f3


def fpknot(m, st, nrint, mg):
    """One more knot in the interval whose residual sum is largest (st.t, st.fpint, st.nrdata, st.n).
    Returns False where no interval can take one (FITPACK reads an unset index there)."""
    t, fpint, nrdata = st.t, st.fpint, st.nrdata
    k = (st.n - nrint - 1) // 2
    fpmax = 0.0
    second = 0.0
    jbegin = 1
    number = 0
    maxpt = maxbeg = 0
    for j in range(1, nrint + 1):
        jpoint = nrdata[j]
        if not (fpmax >= fpint[j]) and jpoint != 0:
            second = fpmax
            fpmax = fpint[j]
            number = j
            maxpt = jpoint
            maxbeg = jbegin
        elif jpoint != 0 and fpint[j] > second:
            second = fpint[j]
        jbegin = jbegin + jpoint + 1
    if number == 0:
        return False
    if fpmax != second:                          # (an exact tie is two halves of one split: the same bits on both sides)
        mg.cmp(fpmax, second, "knot")
    ihalf = maxpt // 2 + 1
    nrx = maxbeg + ihalf
    nxt = number + 1
    for j in range(nxt, nrint + 1):
        jj = nxt + nrint - j
        fpint[jj + 1] = fpint[jj]
        nrdata[jj + 1] = nrdata[jj]
        jk = jj + k
        t[jk + 1] = t[jk]
    nrdata[number] = ihalf - 1
    nrdata[nxt] = maxpt - ihalf
    am = float(maxpt)
    an = float(nrdata[number])
    fpint[number] = _div(fpmax * an, am)
    an = float(nrdata[nxt])
    fpint[nxt] = _div(fpmax * an, am)
    t[nxt + k] = float(nrx - 1)                  # x(nrx), the abscissae being 0 .. m - 1
    st.n += 1
    return True


class State:
    """What one fpcurf call leaves for the next (iopt = 1) and for splev."""

    def __init__(self, m):
        nest = m + K1
        self.m = m
        self.n = 0
        self.t = [0.0] * (nest + 2)
        self.c = [0.0] * (nest + 2)
        self.fpint = [0.0] * (nest + 2)
        self.nrdata = [0] * (nest + 2)
        self.fp = 0.0
        self.ier = 0
        self.iters = 0


def fpcurf(iopt, y, s, st, mg, nest=None, ier_in=0):
    """FITPACK fpcurf, k = 3, w = 1, x = 0 .. m - 1.  y is 1-based.  nest: the knots the caller has
    room for (None: m + 4, all there can be; fewer: ier = 1 where more are needed).  ier_in: what the
    caller's ier holds on entry -- scipy passes the last call's, and a non-zero one makes the first
    knot round of a continued call add one knot whatever nrdata says."""
    m = st.m
    nest = m + K1 if nest is None else nest
    xb, xe = 0.0, float(m - 1)
    t, c, fpint, nrdata = st.t, st.c, st.fpint, st.nrdata
    acc = TOL * s
    nmax = m + K1
    ier = ier_in
    fp0 = fpold = 0.0
    nplus = 0
    st.iters = 0
    a = [[0.0] * (K2 + 1) for _ in range(nmax + 1)]
    g = [[0.0] * (K2 + 2) for _ in range(nmax + 1)]
    b = [[0.0] * (K2 + 1) for _ in range(nmax + 1)]
    q = [[0.0] * (K1 + 1) for _ in range(m + 1)]
    z = [0.0] * (nmax + 1)

    def interp_knots():
        i, j = K2, K // 2 + 2
        for _ in range(m - K1):
            t[i] = float(j - 1)
            i += 1
            j += 1

    restart = True
    if s > 0.0:
        if iopt != 0 and st.n != NMIN:
            fp0 = fpint[st.n]
            fpold = fpint[st.n - 1]
            nplus = nrdata[st.n]
            mg.cmp(fp0, s, "fp0:S")
            restart = not (fp0 > s)
        if restart:
            st.n = NMIN
            fpold = 0.0
            nplus = 0
            nrdata[1] = m - 2
    else:
        st.n = nmax
        if nmax > nest:
            st.ier = 1
            return
        interp_knots()

    fp = fpms = 0.0
    nk1 = 0
    accept = False          # the knots stand (label 250)
    done = False            # label 440
    while not done and not accept:
        again = False
        for _ in range(m):
            n = st.n
            if n == NMIN:
                ier = -2
            nrint = n - NMIN + 1
            nk1 = n - K1
            i = n
            for j in range(1, K1 + 1):
                t[j] = xb
                t[i] = xe
                i -= 1
            fp = 0.0
            for i in range(1, nk1 + 1):
                z[i] = 0.0
                ai = a[i]
                ai[1] = ai[2] = ai[3] = ai[4] = 0.0
            l = K1
            for it in range(1, m + 1):
                xi = float(it - 1)
                yi = y[it]
                while not (xi < t[l + 1] or l == nk1):
                    l += 1
                h = fpbspl(t, xi, l)
                qi = q[it]
                qi[1], qi[2], qi[3], qi[4] = h[1], h[2], h[3], h[4]
                j = l - K1
                for i in range(1, K1 + 1):
                    j += 1
                    piv = h[i]
                    if piv == 0.0:
                        continue
                    aj = a[j]
                    aj[1], cos, sin = fpgivs(piv, aj[1])
                    yi, z[j] = fprota(cos, sin, yi, z[j])
                    if i == K1:
                        break
                    i2 = 1
                    for i1 in range(i + 1, K1 + 1):
                        i2 += 1
                        h[i1], aj[i2] = fprota(cos, sin, h[i1], aj[i2])
                fp = fp + yi * yi
            if ier == -2:
                fp0 = fp
            fpint[n] = fp0
            fpint[n - 1] = fpold
            nrdata[n] = nplus
            fpback(a, z, nk1, K1, c)
            fpms = fp - s
            mg.cmp(abs(fpms), acc, "fpms:acc")
            if abs(fpms) < acc:
                done = True
                break
            mg.cmp(fp, s, "fp:S")
            if fpms < 0.0:
                accept = True
                break
            if n == nmax:
                ier = -1
                done = True
                break
            if n == nest:
                ier = 1
                done = True
                break
            if ier != 0:
                nplus = 1
                ier = 0
            else:
                npl1 = nplus * 2
                rn = float(nplus)
                mg.cmp(fpold - fp, acc, "fpold-fp:acc")
                if fpold - fp > acc:
                    v = _div(rn * fpms, fpold - fp)
                    mg.trunc(v)
                    npl1 = int(v) if v == v and abs(v) < 2147483648.0 else -2147483648
                nplus = min(nplus * 2, max(npl1, nplus // 2, 1))
            fpold = fp
            fpart = 0.0
            i = 1
            l = K2
            new = 0
            for it in range(1, m + 1):
                if not (float(it - 1) < t[l] or l > nk1):
                    new = 1
                    l += 1
                term = 0.0
                l0 = l - K2
                qi = q[it]
                for j in range(1, K1 + 1):
                    l0 += 1
                    term = term + c[l0] * qi[j]
                term = (term - y[it]) * (term - y[it])
                fpart = fpart + term
                if new:
                    store = term * HALF
                    fpint[i] = fpart - store
                    i += 1
                    fpart = store
                    new = 0
            fpint[nrint] = fpart
            for _l in range(nplus):
                if not fpknot(m, st, nrint, mg):
                    ier = 5                      # no interval can take a knot: the fit stands as it is
                    done = True
                    break
                nrint += 1
                if st.n == nmax:
                    interp_knots()
                    again = True                 # (go to 10, then 60: the round count starts again)
                    break
                if st.n == nest:
                    break
            if done or again:
                break
        else:
            accept = True                        # m rounds: fall through to label 250
        if again:
            continue

    if accept and ier != -2:
        n = st.n
        nk1 = n - K1
        fpdisc(t, n, b)
        p1, f1 = 0.0, fp0 - s
        p3, f3 = -1.0, fpms
        p = 0.0
        for i in range(1, nk1 + 1):
            p = p + a[i][1]
        p = _div(float(nk1), p)
        ich1 = ich3 = 0
        n8 = n - NMIN
        h = [0.0] * (K2 + 2)
        for it_p in range(1, MAXIT + 1):
            st.iters = it_p
            pinv = _div(1.0, p)
            for i in range(1, nk1 + 1):
                c[i] = z[i]
                gi, ai = g[i], a[i]
                gi[5] = 0.0
                gi[1], gi[2], gi[3], gi[4] = ai[1], ai[2], ai[3], ai[4]
            for it in range(1, n8 + 1):
                bi = b[it]
                for i in range(1, K2 + 1):
                    h[i] = bi[i] * pinv
                yi = 0.0
                for j in range(it, nk1 + 1):
                    piv = h[1]
                    gj = g[j]
                    gj[1], cos, sin = fpgivs(piv, gj[1])
                    yi, c[j] = fprota(cos, sin, yi, c[j])
                    if j == nk1:
                        break
                    i2 = K1 if j <= n8 else nk1 - j
                    for i in range(1, i2 + 1):
                        i1 = i + 1
                        h[i1], gj[i1] = fprota(cos, sin, h[i1], gj[i1])
                        h[i] = h[i1]
                    h[i2 + 1] = 0.0
            fpback(g, c, nk1, K2, c)
            fp = 0.0
            l = K2
            for it in range(1, m + 1):
                if not (float(it - 1) < t[l] or l > nk1):
                    l += 1
                l0 = l - K2
                term = 0.0
                qi = q[it]
                for j in range(1, K1 + 1):
                    l0 += 1
                    term = term + c[l0] * qi[j]
                fp = fp + (term - y[it]) * (term - y[it])
            fpms = fp - s
            mg.cmp(abs(fpms), acc, "fpms:acc")
            if abs(fpms) < acc:
                break
            if it_p == MAXIT:
                ier = 3
                break
            p2, f2 = p, fpms
            if ich3 == 0:
                mg.cmp(f2 - f3, acc, "f2-f3:acc")
                if not (f2 - f3 > acc):
                    p3, f3 = p2, f2
                    p = p * CON4
                    if p <= p1:
                        p = p1 * CON9 + p2 * CON1
                    continue
                mg.cmp(f2, 0.0)
                if f2 < 0.0:
                    ich3 = 1
            if ich1 == 0:
                mg.cmp(f1 - f2, acc, "f1-f2:acc")
                if not (f1 - f2 > acc):
                    p1, f1 = p2, f2
                    p = _div(p, CON4)
                    if p3 < 0.0:
                        continue
                    if p >= p3:
                        p = p2 * CON1 + p3 * CON9
                    continue
                mg.cmp(f2, 0.0)
                if f2 > 0.0:
                    ich1 = 1
            mg.cmp(f2, f1, "f2:f1")
            mg.cmp(f2, f3, "f2:f3")
            if f2 >= f1 or f2 <= f3:
                ier = 2
                break
            p, p1, f1, p3, f3 = fprati(p1, f1, p2, f2, p3, f3)
    for i in range(st.n - K1 + 1, st.n + 1):     # (the four unused coefficients)
        c[i] = 0.0
    st.fp = fp
    st.ier = ier


def fit(y):
    """The reference's two calls on one track y [m] -> dict(t, c, n, n1, ier1, ier2, iters, fp, S, margin)."""
    y = [float(v) for v in y]
    m = len(y)
    if m < 4:
        raise ValueError("spline_oracle.fit: a clip needs at least 4 frames")
    y1 = [0.0] + y
    st = State(m)
    mg = Margins()
    # scipy gives the first call room for nest = max(m / 2, 8) knots; where that is too few (ier = 1) it
    # continues (iopt = 1) with room for all m + 4, passing the ier = 1 on
    nest = max(m // 2, 2 * K1)
    fpcurf(0, y1, float(m), st, mg, nest)
    if st.ier == 1:
        nest = m + K1
        fpcurf(1, y1, float(m), st, mg, nest, 1)
    n1, ier1, fp1 = st.n, st.ier, st.fp
    t1 = np.array(st.t[1:n1 + 1])
    c1 = np.array(st.c[1:n1 + 1])
    S = span_factor(y)
    fpcurf(1, y1, S, st, mg, nest, st.ier)
    if st.ier == 1:
        fpcurf(1, y1, S, st, mg, m + K1, 1)
    n = st.n
    return dict(t=np.array(st.t[1:n + 1]), c=np.array(st.c[1:n + 1]), n=n, n1=n1, ier1=ier1, ier2=st.ier,
                iters=st.iters, fp=st.fp, fp1=fp1, t1=t1, c1=c1, S=S, margin=mg.m, margin_at=mg.what)


def fresh_fit(y, s):
    """One iopt = 0 call with smoothing factor s (what the continuation must NOT be mistaken for)."""
    y = [float(v) for v in y]
    st = State(len(y))
    fpcurf(0, [0.0] + y, float(s), st, Margins(), max(len(y) // 2, 2 * K1))
    if st.ier == 1:
        fpcurf(1, [0.0] + y, float(s), st, Margins(), len(y) + K1, 1)
    return dict(t=np.array(st.t[1:st.n + 1]), c=np.array(st.c[1:st.n + 1]), n=st.n, ier=st.ier, fp=st.fp)


def splev(t, c, x):
    """s(x) by splev's arithmetic (ext = 0: the end pieces extrapolate); t, c [n], x any shape."""
    t = [0.0] + [float(v) for v in t]
    c = [0.0] + [float(v) for v in c]
    n = len(t) - 1
    nk1 = n - K1
    out = np.empty(np.shape(x), np.float64)
    flat = out.reshape(-1)
    l = K1
    l1 = l + 1
    for idx, arg in enumerate(np.asarray(x, np.float64).reshape(-1).tolist()):
        while not (arg >= t[l] or l1 == K2):
            l1 = l
            l -= 1
        while not (arg < t[l1] or l == nk1):
            l = l1
            l1 = l + 1
        h = fpbspl(t, arg, l)
        sp = 0.0
        ll = l - K1
        for j in range(1, K1 + 1):
            ll += 1
            sp = sp + c[ll] * h[j]
        flat[idx] = sp
    return out


def resample(y, R):
    """fit(y) and its samples at j * (1.0 / R), j = 0 .. R * m - 1."""
    f = fit(y)
    step = 1.0 / R
    f["xr"] = splev(f["t"], f["c"], np.arange(R * len(y), dtype=np.float64) * step)
    return f


INFO_FIELDS = ("n1", "n", "ier1", "ier2", "iters")


def info_record(f):
    """The kernel's info record of a fit: n after stage 1, n after stage 2, ier of each stage, p iterations."""
    return np.array([f[k] for k in INFO_FIELDS], np.int32)
