"""The fit reduction (fit_reduce_kernel of unconfined_amd/csrc/ucf_fit.hip) restated in numpy from its documented arithmetic
(ucf_fit.hip, ucf_fit.h and ucf_debug_fit_reduce of include/ucf.h), one rounded fp64 operation at a time, vectorised over the
256 lanes of a pass; the synthetic inputs that tests/test_fit_reduce_restate.py (CPU) and tests/test_gpu_fit_reduce_edges.py
(GPU) share; and the call of ucf_debug_fit_reduce.  A helper module: no tests here.

An input set is a dict: source (0 slots, 1 network, 2 field), npar, nsets, nobs, two_dlog, h, dh (None: no derivative data), Hc
[nplans], obs, w, dobs, wd [nobs]; slots: slot [nobs], plan_stride; network: prefix, stride, at, count [nobs]; field: the same
four and q, tfac per term, first [nobs + 1]."""
import numpy as np

from unconfined_amd.abi import FIT_FIELD as FIELD, FIT_NETWORK as NETWORK, FIT_SLOTS as SLOTS

SOURCES = {"slots": SLOTS, "network": NETWORK, "field": FIELD}
LANES, WAVE = 256, 64
SENTINEL = -999999.9
COUNTS = (1, 2, 3, 5, 32)          # depths of a ref: 2 is where the loop of network_h runs no iteration, 32 is UCF_MAX_NZ
ORDERS = ("documented", "ascending", "waves_reversed", "butterfly_up")


def nsums(npar, deriv):
    return 1 + npar + npar * (npar + 1) // 2 + (1 if deriv else 0)


# ---- the sources

def network_h(h, prefix, stride, at, count, nplans, plan):
    """count == 1: the value itself; otherwise s = v[1]; s = s + v[j], j = 2 .. n-1; ((v[0] + 2.0 * s) + v[n-1]) / (2 n)"""
    base = prefix * np.int64(nplans) + np.int64(plan) * stride + at
    out = np.empty(len(base))
    for n in np.unique(count):
        m = count == n
        b = base[m]
        if n == 1:
            out[m] = h[b]
            continue
        s = h[b + 1]
        for j in range(2, int(n)):
            s = s + h[b + j]
        out[m] = ((h[b] + 2.0 * s) + h[b + int(n) - 1]) / np.float64(2 * int(n))
    return out


def source_value(inp, h, plan, derivative):
    """the dimensionless value of every observation under `plan`, from h (derivative: from dh, a field term scaled by its tfac)"""
    if inp["source"] == SLOTS:
        return h[np.int64(plan) * inp["plan_stride"] + inp["slot"].astype(np.int64)]
    nplans = inp["nsets"] * (1 + 2 * inp["npar"])
    v = network_h(h, inp["prefix"], inp["stride"], inp["at"].astype(np.int64), inp["count"], nplans, plan)
    if inp["source"] == NETWORK:
        return v
    if derivative:
        v = inp["tfac"] * v
    p = inp["q"] * v
    first = inp["first"].astype(np.int64)
    nterm = np.diff(first)
    acc = np.zeros(inp["nobs"])                      # acc = +0.0: what an observation without terms stays
    for k in range(int(nterm.max()) if len(nterm) else 0):
        m = nterm > k
        acc[m] = acc[m] + p[first[:-1][m] + k]
    return acc


# ---- the reduction

def reduce_lanes(v, order):
    """v [nsum][256] per-lane partial sums -> [nsum]: the butterfly v = v + v[lane ^ m], m = 32 .. 1, per wave of 64 lanes, then
    wave 0 + 1 + 2 + 3 in that order (or one of the changed orders that the CPU tests tell apart)"""
    lane = np.arange(LANES)
    for m in ((1, 2, 4, 8, 16, 32) if order == "butterfly_up" else (32, 16, 8, 4, 2, 1)):
        v = v + v[:, lane ^ m]
    part = [v[:, k * WAVE] for k in range(LANES // WAVE)]
    if order == "waves_reversed":
        part = part[::-1]
    out = part[0]
    for p in part[1:]:
        out = out + p
    return out


def restate(inp, order="documented"):
    """dict of sums [nsets][nsums], nbad [nsets], J [nsets][nobs][npar], sim [nplans][nobs] and, with dh, Jd, simd; also the
    terms of every sum (`terms`, `terms_d` [nsets][nsums][nobs], `counted`, `weighted` [nsets][nobs]) for the longdouble check"""
    npar, nsets, nobs = inp["npar"], inp["nsets"], inp["nobs"]
    deriv = inp["dh"] is not None
    P, NS = 1 + 2 * npar, nsums(npar, deriv)
    two_dlog = np.float64(inp["two_dlog"])
    w, obs = inp["w"], inp["obs"]
    out = dict(sums=np.zeros((nsets, NS)), nbad=np.zeros(nsets, np.int32), J=np.zeros((nsets, nobs, npar)), sim=np.zeros((nsets * P, nobs)),
               terms=np.zeros((nsets, NS, nobs)), terms_d=np.zeros((nsets, NS, nobs)), counted=np.zeros((nsets, nobs), bool),
               weighted=np.zeros((nsets, nobs), bool))
    if deriv:
        out.update(Jd=np.zeros((nsets, nobs, npar)), simd=np.zeros((nsets * P, nobs)))
    with np.errstate(all="ignore"):
        for s in range(nsets):
            def side(h, derivative, wt, target):
                """s[k], d[j], and the terms phi | g | A of one curve: wr = wt * (target - s[0]), wd[j] = wt * d[j]"""
                sv = np.stack([source_value(inp, h, s * P + k, derivative) * inp["Hc"][s * P + k] for k in range(P)])
                d = [(sv[1 + 2 * j] - sv[2 + 2 * j]) / two_dlog for j in range(npar)]
                wr = wt * (target - sv[0])
                wd = [wt * d[j] for j in range(npar)]
                t = [wr * wr] + [wd[j] * wr for j in range(npar)] + [wd[j] * wd[k] for j in range(npar) for k in range(j, npar)]
                return sv, d, t
            sv, d, t = side(inp["h"], False, w, obs)
            out["sim"][s * P:(s + 1) * P] = sv
            out["J"][s] = np.stack(d, axis=1) if npar else np.zeros((nobs, 0))
            ok = np.isfinite(sv).all(axis=0)
            t1 = np.zeros((NS, nobs))
            t1[:len(t)] = t
            t2, active = np.zeros((NS, nobs)), np.zeros(nobs, bool)
            if deriv:
                sd, dd, td = side(inp["dh"], True, inp["wd"], inp["dobs"])
                out["simd"][s * P:(s + 1) * P] = sd
                out["Jd"][s] = np.stack(dd, axis=1) if npar else np.zeros((nobs, 0))
                ok = ok & ((inp["wd"] == 0.0) | np.isfinite(sd).all(axis=0))
                active = inp["wd"] > 0.0
                t2[:len(td)] = td
                t2[NS - 1] = td[0]                   # phi_d += wrd * wrd
            out["nbad"][s] = int((~ok).sum())
            out["terms"][s], out["terms_d"][s], out["counted"][s], out["weighted"][s] = t1, t2, ok, ok & active
            if order == "ascending":                 # a changed order: one accumulator over the observations as they come
                acc = np.zeros(NS)
                for i in np.flatnonzero(ok):
                    acc[:len(t)] = acc[:len(t)] + t1[:len(t), i]
                    if active[i]:
                        acc = acc + t2[:, i]
                out["sums"][s] = acc
                continue
            acc = np.zeros((NS, LANES))
            for i0 in range(0, nobs, LANES):         # lane l takes l, l + 256, ... in ascending order
                n = min(LANES, nobs - i0)
                sl = slice(i0, i0 + n)
                a = acc[:, :n]
                a[:len(t)] = np.where(ok[sl], a[:len(t)] + t1[:len(t), sl], a[:len(t)])
                # the derivative term: skipped, not added as zero, where it has no weight
                acc[:, :n] = np.where(ok[sl] & active[sl], a + t2[:, sl], a)
            out["sums"][s] = reduce_lanes(acc, order)
    return out


def longdouble_sums(inp, res, s, start="rounded"):
    """(sums, sum|terms|) of set s in np.longdouble over the observations that count.  start = "rounded": from the residual
    r = obs - s[0] and the Jacobian d[j] as fp64 holds them (J is an output of the kernel in its own right; jacobian_error holds
    it to the longdouble value); start = "sim": from the sim / simd rows, r and d formed in longdouble too"""
    L = np.longdouble
    npar = inp["npar"]

    def side(rows, jac, wt, target, keep):
        if start == "sim":
            sv = rows.astype(L)
            d = [(sv[1 + 2 * j] - sv[2 + 2 * j]) / L(inp["two_dlog"]) for j in range(npar)]
            r = target.astype(L) - sv[0]
        else:
            with np.errstate(all="ignore"):
                d, r = [jac[:, j].astype(L) for j in range(npar)], (target - rows[0]).astype(L)
        wr = wt.astype(L) * r
        wd = [wt.astype(L) * d[j] for j in range(npar)]
        t = [wr * wr] + [wd[j] * wr for j in range(npar)] + [wd[j] * wd[k] for j in range(npar) for k in range(j, npar)]
        return np.stack(t)[:, keep]
    P = 1 + 2 * npar
    t = side(res["sim"][s * P:(s + 1) * P], res["J"][s], inp["w"], inp["obs"], res["counted"][s])
    tot, mag = t.sum(axis=1), np.abs(t).sum(axis=1)
    if inp["dh"] is not None:
        td = side(res["simd"][s * P:(s + 1) * P], res["Jd"][s], inp["wd"], inp["dobs"], res["weighted"][s])
        tot, mag = tot + td.sum(axis=1), mag + np.abs(td).sum(axis=1)
        tot, mag = np.append(tot, td[0].sum()), np.append(mag, np.abs(td[0]).sum())
    return tot, mag


def jacobian_error(inp, res, s):
    """worst |d - (s+ - s-) / two_dlog| / (u |that|) over the finite entries of J (and Jd) of set s, the quotient in np.longdouble"""
    L = np.longdouble
    P, worst = 1 + 2 * inp["npar"], 0.0
    for rows, jac in ((res["sim"], res["J"]), (res.get("simd"), res.get("Jd"))):
        for j in range(inp["npar"] if rows is not None else 0):
            sv = rows[s * P:(s + 1) * P].astype(L)
            with np.errstate(all="ignore"):
                ref = (sv[1 + 2 * j] - sv[2 + 2 * j]) / L(inp["two_dlog"])
            m = np.isfinite(ref) & (ref != 0)
            assert (np.isfinite(jac[s][:, j]) == np.isfinite(ref)).all()
            if m.any():
                worst = max(worst, float((np.abs(jac[s][:, j][m].astype(L) - ref[m]) / np.abs(ref[m])).max() / 2.0 ** -53))
    return worst


# ---- synthetic inputs

KINDS = {1: "base value NaN", 2: "one perturbed plan +Inf", 3: "w = 0", 4: "wd = 0, every sd[k] and dobs NaN", 5: "wd > 0, one sd[k] not finite",
         6: "wd > 0 and w = 0", 7: "the Wynn sentinel", 9: "wd = 0, dobs NaN, sd finite", 10: "wd = 0"}          # every other i % 12: plain


def ragged_refs(n, nplans):
    """n refs in three groups (ref k in group k % 3) with different prefix and stride, a nonzero at, counts from COUNTS in turn; no
    two refs share a double.  Returns prefix, stride, at, count and the length of h"""
    group, count = np.arange(n) % 3, np.array(COUNTS, np.int32)[(np.arange(n) // 3) % len(COUNTS)]
    at, stride = np.zeros(n, np.int32), np.zeros(3, np.int64)
    for g in range(3):
        k = np.flatnonzero(group == g)
        start = g + 1 + np.concatenate([[0], np.cumsum(count[k])])
        at[k] = start[:-1]
        stride[g] = start[-1] + 2 + 40 * g           # a tail that no ref reads; the three strides differ
    prefix = np.concatenate([[0], np.cumsum(stride)])[:3]
    return prefix[group].astype(np.int64), stride[group].astype(np.int64), at, count, int(stride.sum()) * nplans


def expected_bad(source, npar, deriv, nobs, nterm=None):
    """the observations that the counting rule excludes, from the pattern of kinds alone: base NaN; one perturbed plan +Inf
    (there is none with npar = 0); with derivative data a weighted derivative that is not finite.  A field observation without
    terms is +0.0 under every plan and always counts."""
    kind = np.arange(nobs) % 12
    bad = (kind == 1) | ((kind == 2) & (npar > 0)) | ((kind == 5) & bool(deriv))
    if nterm is not None:
        bad &= nterm > 0
    return bad


def orders_differ(inp):
    """whether the data tell the documented order from every changed one: the bytes of phi differ, and those of the upper
    triangle of A where there is one"""
    npar = inp["npar"]
    doc = restate(inp)["sums"]
    A = slice(1 + npar, 1 + npar + npar * (npar + 1) // 2)
    for order in ORDERS[1:]:
        alt = restate(inp, order)["sums"]
        if alt[:, 0].tobytes() == doc[:, 0].tobytes() or (npar and alt[:, A].tobytes() == doc[:, A].tobytes()):
            return False
    return True


# Two orders of a sum of positive terms (phi, a diagonal entry of A) that differ only in their last additions -- the waves in
# reverse, the butterfly upward -- round to the same double more often than not, whatever the data (measured on these inputs:
# two times in three per parameter set).  The cases with a second pass whose draw 0 does not tell every changed order apart take
# the first draw that does (found with orders_differ; tests/test_fit_reduce_restate.py holds every case to it):
# (source, npar, deriv, nobs) -> draw
DRAWS = {
    (0, 0, 0, 300): 1, (0, 0, 0, 513): 9, (0, 0, 0, 1025): 22, (0, 0, 1, 257): 5, (0, 0, 1, 300): 5, (0, 0, 1, 513): 3, (0, 0, 1, 1025): 7,
    (0, 1, 0, 257): 5, (0, 1, 0, 300): 5, (0, 1, 0, 513): 1, (0, 1, 0, 1025): 21, (0, 1, 1, 300): 36, (0, 1, 1, 513): 6, (0, 1, 1, 1025): 36,
    (0, 2, 0, 257): 5, (0, 3, 0, 257): 6, (0, 3, 1, 257): 1, (0, 4, 0, 513): 2, (0, 4, 1, 300): 2, (0, 4, 1, 513): 9, (0, 4, 1, 1025): 2,
    (0, 5, 0, 257): 1, (0, 5, 1, 257): 2, (0, 6, 0, 257): 1, (0, 7, 1, 257): 1, (0, 8, 0, 257): 3, (0, 8, 0, 513): 6, (0, 8, 0, 1025): 3,
    (0, 8, 1, 257): 2, (0, 8, 1, 300): 7, (0, 8, 1, 513): 1, (0, 8, 1, 1025): 4, (1, 0, 0, 257): 1, (1, 0, 0, 300): 14, (1, 0, 0, 1025): 9,
    (1, 0, 1, 257): 7, (1, 0, 1, 513): 2, (1, 0, 1, 1025): 1, (1, 1, 0, 257): 2, (1, 1, 0, 300): 12, (1, 1, 0, 513): 21, (1, 1, 1, 257): 1,
    (1, 1, 1, 300): 2, (1, 1, 1, 513): 9, (1, 1, 1, 1025): 14, (1, 2, 0, 257): 1, (1, 2, 1, 257): 1, (1, 3, 0, 257): 1, (1, 4, 0, 257): 2,
    (1, 4, 0, 300): 1, (1, 4, 0, 513): 3, (1, 4, 0, 1025): 2, (1, 4, 1, 300): 1, (1, 4, 1, 513): 2, (1, 4, 1, 1025): 1, (1, 5, 0, 257): 5,
    (1, 7, 1, 257): 3, (1, 8, 0, 257): 2, (1, 8, 0, 300): 2, (1, 8, 0, 513): 10, (1, 8, 0, 1025): 5, (1, 8, 1, 300): 3, (1, 8, 1, 513): 3,
    (2, 0, 0, 257): 1, (2, 0, 0, 300): 2, (2, 0, 0, 513): 2, (2, 0, 0, 1025): 2, (2, 0, 1, 300): 13, (2, 0, 1, 513): 2, (2, 1, 0, 257): 5,
    (2, 1, 0, 300): 2, (2, 1, 0, 513): 25, (2, 1, 1, 257): 2, (2, 1, 1, 300): 4, (2, 1, 1, 513): 5, (2, 1, 1, 1025): 4, (2, 2, 0, 257): 1,
    (2, 2, 1, 257): 1, (2, 4, 0, 257): 4, (2, 4, 0, 513): 5, (2, 4, 0, 1025): 7, (2, 4, 1, 300): 4, (2, 4, 1, 513): 3, (2, 4, 1, 1025): 1,
    (2, 5, 0, 257): 1, (2, 5, 1, 257): 4, (2, 7, 0, 257): 2, (2, 8, 0, 300): 1, (2, 8, 0, 513): 10, (2, 8, 0, 1025): 1, (2, 8, 1, 300): 1,
    (2, 8, 1, 513): 4,
}


def synthetic(source, npar, deriv, nobs, nsets):
    """the input set of a case, from a generator seeded by (source, npar, deriv, nobs) and the draw that DRAWS gives them.
    Observation i is of kind i % 12 (KINDS); a value is made NaN / Inf / the sentinel in the first double that the observation
    reads under the plan in question"""
    rng = np.random.default_rng([source, npar, int(deriv), nobs, DRAWS.get((source, npar, int(deriv), nobs), 0)])
    P = 1 + 2 * npar
    nplans = nsets * P
    inp = dict(source=source, npar=npar, nsets=nsets, nobs=nobs, two_dlog=2.0e-3, dh=None, dobs=None, wd=None)
    if source == SLOTS:
        inp["plan_stride"] = nobs + 3
        inp["slot"] = rng.permutation(nobs + 3)[:nobs].astype(np.int32)
        nh = nplans * inp["plan_stride"]
        cell = lambda plan: np.int64(plan) * inp["plan_stride"] + inp["slot"]
        nterm = None
    else:
        if source == NETWORK:
            nref, nterm = nobs, None
            head = np.arange(nobs)
        else:
            i = np.arange(nobs)
            nterm = np.array([1, 2, 3, 7])[(i // 12 + i) % 4]
            nterm[(i % 12 == 8) | (i % 24 == 12)] = 0
            inp["first"] = np.concatenate([[0], np.cumsum(nterm)]).astype(np.int32)
            nref = int(inp["first"][-1])
            head = np.minimum(inp["first"][:-1], max(nref - 1, 0))               # first term (not used where there is none)
            inp["q"] = rng.choice(np.array([-1.0, 1.0, 1.0]), nref) * 10.0 ** rng.uniform(-1.0, 1.0, nref)      # negative: image wells
            inp["tfac"] = np.where(np.arange(nref) % 3 == 0, 1.0, 1.0 / (1.0 - rng.uniform(0.0, 0.9, nref)))
        inp["prefix"], inp["stride"], inp["at"], inp["count"], nh = ragged_refs(nref, nplans)
        nh = max(nh, 1)
        if nref:
            cell = lambda plan: (inp["prefix"] * nplans + np.int64(plan) * inp["stride"] + inp["at"])[head]
        else:
            cell = lambda plan: np.zeros(nobs, np.int64)
    # Every value that observation i reads, and its obs and dobs, have the magnitude scale_i, log-uniform over six decades (the
    # sentinel's for kind 7), and its weights 1 / scale_i: the TERMS of a sum are then of one magnitude, every addition rounds
    # at the scale of the result, and the order of the additions shows in its bits.  (With terms over twelve decades a sum is
    # two or three of them and most orders agree.)
    scale = 10.0 ** rng.uniform(-3.0, 3.0, nobs)
    scale[np.arange(nobs) % 12 == 7] = 1.0e6
    owner = np.full(nh, -1)
    for plan in range(nplans):
        if source == SLOTS:
            owner[cell(plan)] = np.arange(nobs)
        elif nref:
            base = inp["prefix"] * nplans + np.int64(plan) * inp["stride"] + inp["at"]
            depth = np.arange(int(inp["count"].sum())) - np.repeat(np.cumsum(inp["count"]) - inp["count"], inp["count"])
            owner[np.repeat(base, inp["count"]) + depth] = np.repeat(np.arange(nobs) if nterm is None else np.repeat(np.arange(nobs), nterm), inp["count"])
    size = np.where(owner >= 0, scale[np.maximum(owner, 0)], 1.0)
    mixed = lambda n: rng.choice(np.array([-1.0, 1.0]), n) * rng.uniform(0.5, 2.0, n)
    h, dh = size * mixed(nh), size * mixed(nh)
    inp["Hc"] = rng.uniform(0.5, 2.0, nplans)
    inp["obs"], inp["w"] = scale * mixed(nobs), rng.uniform(0.5, 1.5, nobs) / scale
    dobs, wd = scale * mixed(nobs), rng.uniform(0.5, 1.5, nobs) / scale
    i = np.arange(nobs)
    kind = i % 12
    has = np.ones(nobs, bool) if nterm is None else nterm > 0
    inp["w"][(kind == 3) | (kind == 6)] = 0.0
    wd[(kind == 4) | (kind == 9) | (kind == 10)] = 0.0
    dobs[(kind == 4) | (kind == 9)] = np.nan
    for s in range(nsets):
        p0 = s * P
        m = has & (kind == 1)
        h[cell(p0)[m]] = np.nan
        m = has & (kind == 7)
        h[cell(p0)[m]] = SENTINEL
        for k in range(P):
            m = has & (kind == 4)
            dh[cell(p0 + k)[m]] = np.nan
            if k >= 1:                               # every perturbed plan is hit over a case that is long enough
                m = has & (kind == 2) & (1 + (i // 12) % max(2 * npar, 1) == k)
                h[cell(p0 + k)[m]] = np.inf
            m = has & (kind == 5) & ((i // 12) % P == k)
            dh[cell(p0 + k)[m]] = (np.nan, np.inf, -np.inf)[k % 3]
    inp["h"] = h
    if deriv:
        inp.update(dh=dh, dobs=dobs, wd=wd)
    return inp, nterm


# ---- the hook

def addr(a):
    return None if a is None else a.ctypes.data


def debug_fit_reduce(inp, want=("J", "sim", "Jd", "simd")):
    """ucf_debug_fit_reduce on an input set: dict of sums, nbad and the arrays of `want` that the call can give"""
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    npar, nsets, nobs = inp["npar"], inp["nsets"], inp["nobs"]
    deriv = inp.get("dh") is not None
    f64 = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.float64)
    i32 = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.int32)
    i64 = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.int64)
    a = {k: f64(k) for k in ("h", "dh", "Hc", "obs", "w", "dobs", "wd", "q", "tfac")}
    a.update({k: i32(k) for k in ("slot", "at", "count", "first")})
    a.update({k: i64(k) for k in ("prefix", "stride")})
    nplans = max(nsets, 0) * (1 + 2 * max(npar, 0))
    out = dict(sums=np.full((max(nsets, 0), nsums(max(npar, 0), deriv)), -7.0), nbad=np.full(max(nsets, 0), -7, np.int32))
    shapes = dict(J=(nsets, nobs, npar), Jd=(nsets, nobs, npar), sim=(nplans, nobs), simd=(nplans, nobs))
    for k in want:
        if deriv or k in ("J", "sim"):
            out[k] = np.full(tuple(max(n, 0) for n in shapes[k]), -7.0)
    nref = inp["nref"] if "nref" in inp else (0 if a["prefix"] is None else len(a["prefix"]))
    ucflib.check(so.ucf_debug_fit_reduce(inp["source"], npar, nsets, nobs, float(inp["two_dlog"]), inp.get("nh", len(a["h"])), addr(a["h"]), addr(a["dh"]),
                                         addr(a["Hc"]), addr(a["obs"]), addr(a["w"]), addr(a["dobs"]), addr(a["wd"]), addr(a["slot"]),
                                         int(inp.get("plan_stride", 0)), nref, addr(a["prefix"]), addr(a["stride"]), addr(a["at"]), addr(a["count"]),
                                         addr(a["q"]), addr(a["tfac"]), addr(a["first"]), addr(out["sums"]), addr(out["nbad"]), addr(out.get("J")),
                                         addr(out.get("sim")), addr(out.get("Jd")), addr(out.get("simd"))))
    return out
