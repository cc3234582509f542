"""The learner's arithmetic kernels (csrc/rl_kernels.hip from hab_compute_returns down) against float64 references written here from
the definitions in include/habitat_amd.h and oracle/functional.py: hab_compute_returns (both variants), hab_advantages (modes 0-4 and
the 2 -> 4 -> 3 sequence on one aliased stats buffer), hab_ppo_loss / hab_ppo_loss_ver, hab_clip_adam_step, hab_lagrange_adam_step,
hab_ver_compute_returns, hab_ver_is_coeffs and hab_sample_actions, at the smallest shapes where each code path changes.

Every GPU case: outputs are pre-filled with NaN (a sentinel for integers) inside guard elements, everything the entry point is not
documented to write must come back bit for bit, and every call is made twice on fresh copies and must reproduce its bits.

Error bars.  Hyper-parameters cross the C ABI as float, so the references use the float32-rounded value widened to double.  Results the
code forms with _rn operations in the reference's order (GAE variant 0, raw advantages, importance coefficients, sampling), integers
and copies are compared bitwise.  Everything else gets a per-element allowance computed in float64 from the operands by running error
analysis (class R below): each float32 operation of the kernel adds OP |result| to the bound it inherits from its operands, which is
the k 2^-24 (magnitude sum) form with the magnitudes taken where the roundings happen.  OP is one ulp, 2 x 2^-24: an operation may round
faithfully (a contracted multiply-add, a division or square root that is not correctly rounded), and a round-to-nearest evaluation
then sits within half of the allowance, which is what the CPU self-checks ask for.  expf, powf and rsqrtf are allowed 2 ulp each; sums
get (adds on the longest path) x OP x sum |term|; the GAE recurrences carry their own bound on |values|.
The count k of roundings is stated next to each reference.  The unmarked CPU tests hold a float32 evaluation of every case (oracle /
torch arithmetic) to HALF of the allowance, and show that each plausible wrong reference EXCEEDS it on these inputs.

One listed wrong variant cannot be caught by any finite input and is pinned instead (test_tie_weight_is_unobservable): the surrogate
terms tie outside the clip range only where adv == 0, and there d_logp = -adv * w * ratio / B is zero for every tie weight w.

hab_advantages with exactly one finite entry divides by max(C - 1, 1) where torch.var_mean gives NaN; that divergence is not tested.

The hyper-parameters are rounded BEFORE 1 - beta is formed: the kernels' 1 - float(0.999) is 1.3e-5 relative (216 x 2^-24) away from
torch.optim.Adam's float(1 - 0.999).  That is the C ABI's contract, so the float32 self-checks hand the oracle the rounded values.
torch's float32 vector_norm is hundreds of allowances off at n = 2^21 (the kernel sums its squares in double), so the self-check of the
norm sums in double too.

Worst error / allowance seen on the MI355X (printed at the end of a GPU run with -s); no case came above 0.5:
  hab_compute_returns    exact 0.325 (and the bits of the float32 CPU loop), scan 0.102
  hab_advantages         adv 0.203, adv after 2-4-3 0.203, stats mean 0.152, var 0.058, count exact; raw adv bitwise
  hab_ppo_loss           d_value 0.253, d_logp 0.228, d_entropy 0.203, out[0..3] 0.054, out[4..9] 0.168, out[10], out[11] exact
  hab_ppo_loss_ver       d_value 0.314, d_logp 0.242, d_entropy 0.360, out[0..3] 0.054, out[4..9] 0.168, out[13..19] 0.044 (minima,
                         maxima and the two count-based means exact), out[20], out[21] 0.120
  hab_clip_adam_step     params 0.499, exp_avg 0.450, exp_avg_sq 0.327, grad_norm 0.176
  hab_lagrange_adam_step log_alpha 0.362, exp_avg 0.092, exp_avg_sq 0.156, alpha_out 0.134
  hab_ver_compute_returns  every element bit-equal to the rounded float64 loop (one float32 ulp is allowed)
  hab_ver_is_coeffs, hab_sample_actions  bitwise
"""
import ctypes as C
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from habitat_amd import _lib
from habitat_amd.rl.ver.ver_rollout_storage import pack_info_from_ids_np
from oracle import functional as O

gpu = pytest.mark.gpu
U = 2.0 ** -24
OP = 2 * U             # what one float32 operation may add: one ulp, a faithful rounding (see the module docstring)
NAN = float("nan")
HAB_ERR_ARG = -1
G = 4                  # guard elements on each side of every output (4 floats keep the 16-byte alignment)
ISENT = -77            # guard / pre-fill of integer outputs
WORST = {}             # entry point / output -> worst error / allowance seen in this GPU run
f32, f64 = np.float32, np.float64


def w32(x):
    """A hyper-parameter as the kernel receives it: rounded to float32, widened to double."""
    return float(np.float32(x))


def cdiv(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def L():
    yield _lib.lib()
    for k in sorted(WORST):
        print("worst error/allowance %-58s %.3f" % (k, WORST[k]))


_KEEP = []


def P(t):
    """Device pointer of a tensor for a ctypes call (kept alive until the caller has synchronised)."""
    if t is None:
        return None
    _KEEP.append(t)
    if len(_KEEP) > 96:
        del _KEEP[:48]
    return C.c_void_p(t.data_ptr())


def PB(t, off=G):
    """Pointer to the body of a guarded storage."""
    _KEEP.append(t)
    return C.c_void_p(t.data_ptr() + off * t.element_size())


S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def T(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def dev(x):
    return T(x).cuda()


def guard(x, fill=NAN):
    x = T(x).reshape(-1)
    s = torch.full((x.numel() + 2 * G,), fill, dtype=x.dtype)
    s[G:G + x.numel()] = x
    return s


def body(s):
    return s[G:s.numel() - G]


def nans(n):
    return torch.full((n,), NAN)


def bits(t):
    t = T(t).contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def same_f32(got, exp):
    """Bitwise, except that any NaN matches any NaN (a NaN produced by arithmetic has no promised payload)."""
    got, exp = T(got).reshape(-1), T(exp).reshape(-1)
    n = torch.isnan(exp)
    return torch.equal(torch.isnan(got), n) and torch.equal(bits(got)[~n], bits(exp)[~n])


def untouched(init, got, written=None):
    """Guards, and every body element outside `written`, still hold the bits they had before the call."""
    keep = torch.ones(init.numel(), dtype=torch.bool)
    if written is not None:
        keep[G:init.numel() - G] = ~T(np.asarray(written)).reshape(-1)
    return torch.equal(bits(init)[keep], bits(got)[keep])


def twice(run):
    a, b = run(), run()
    for k in a:
        assert same_bits(a[k], b[k]), f"{k}: two runs on fresh copies differ"
    return a


def ratio_of(got, ref, allow):
    """Worst |got - ref| / allow.  inf where the NaN or infinity pattern differs or where allow == 0 and got != ref."""
    got, ref, allow = np.broadcast_arrays(np.asarray(got, f64), np.asarray(ref, f64), np.asarray(allow, f64))
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return math.inf
    inf = ~nan & np.isinf(ref)
    if not np.array_equal(got[inf], ref[inf]):
        return math.inf
    fin = ~nan & ~inf
    if np.isinf(got[fin]).any():
        return math.inf
    err, a = np.abs(got[fin] - ref[fin]), allow[fin]
    if (err[~(a > 0)] != 0).any():
        return math.inf
    nz = a > 0
    return float((err[nz] / a[nz]).max()) if nz.any() else 0.0


def hold(name, got, r):
    """GPU result against a reference R: within the allowance, worst ratio recorded."""
    q = ratio_of(T(got).numpy() if isinstance(got, torch.Tensor) else got, r.v, r.e)
    WORST[name] = max(WORST.get(name, 0.0), q)
    assert q <= 1.0, f"{name}: error is {q:.3g} x the allowance"


def half(name, got, r):
    """CPU float32 evaluation against a reference R: within HALF of the allowance (the bar can be met at all)."""
    q = ratio_of(T(got).detach().numpy() if isinstance(got, torch.Tensor) else got, r.v, r.e)
    assert q <= 0.5, f"{name}: the float32 evaluation on the CPU is at {q:.3g} x the allowance"


def caught(got, r):
    return ratio_of(got.v if isinstance(got, R) else got, r.v, r.e) > 1.0


# ------------------------------------------------------------------------------------------------
# Running error analysis: v is the float64 value, e bounds |float32 result - v| to first order.  Every operation takes the number k of
# float32 roundings it stands for (0: done in double by the kernel, or exact).
# ------------------------------------------------------------------------------------------------
class R:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, f64)
        self.e = np.zeros_like(self.v) + e

    def __getitem__(self, i):
        return R(self.v[i], self.e[i])


TINY = 1e-300


def _r(x):
    return x if isinstance(x, R) else R(x)


def rnd(v, e=0.0, k=1):
    v = np.asarray(v, f64)
    return R(v, e + k * OP * np.abs(v))


def add(a, b, k=1):
    a, b = _r(a), _r(b)
    return rnd(a.v + b.v, a.e + b.e, k)


def sub(a, b, k=1):
    a, b = _r(a), _r(b)
    return rnd(a.v - b.v, a.e + b.e, k)


def mul(a, b, k=1):
    a, b = _r(a), _r(b)
    return rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, k)


def div(a, b, k=1):
    a, b = _r(a), _r(b)
    q = a.v / b.v
    return rnd(q, (a.e + np.abs(q) * b.e) / np.maximum(np.abs(b.v) - b.e, TINY), k)


def neg(a):
    return R(-a.v, a.e)


def sqrt_(a, k=1):
    s = np.sqrt(a.v)
    return rnd(s, np.maximum(s - np.sqrt(np.maximum(a.v - a.e, 0.0)), np.sqrt(a.v + a.e) - s), k)


def exp_(a, ulps=2):
    v = np.exp(a.v)
    return rnd(v, v * np.expm1(a.e), ulps)


def rsqrt_(a, ulps=2):
    v = 1.0 / np.sqrt(a.v)
    return rnd(v, 0.5 * v * a.e / np.maximum(a.v - a.e, TINY), ulps)


def min_(a, b):
    a, b = _r(a), _r(b)
    return R(np.minimum(a.v, b.v), np.maximum(a.e, b.e))


def max_(a, b):
    a, b = _r(a), _r(b)
    return R(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def where_(c, a, b):
    a, b = _r(a), _r(b)
    return R(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def _key(s):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(s))


# ================================================================================================
# hab_compute_returns
# ================================================================================================
GAMMA, TAU = 0.99, 0.95
GAE_T = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
GAE_N = (1, 3, 64, 65)
GAE_SHAPES = sorted({(t, 3) for t in GAE_T} | {(65, n) for n in GAE_N} | {(0, 1), (0, 65), (200, 1), (200, 65)})
PATTERNS = ("rand", "ones", "zeros", "endT", "borders")


@functools.lru_cache(maxsize=None)
def gae_data(Tn, N, pattern):
    g = rng(1, Tn, N, _key(pattern))
    r = g.standard_normal((Tn + 1, N)).astype(f32)
    v = (2.0 * g.standard_normal((Tn + 1, N))).astype(f32)
    r[Tn] = NAN          # never read
    v[Tn] = NAN          # overwritten from next_value under GAE, never read otherwise
    if pattern == "rand":
        m = g.random((Tn + 1, N)) > 0.1
    elif pattern == "zeros":
        m = np.zeros((Tn + 1, N), bool)
    else:
        m = np.ones((Tn + 1, N), bool)
        if pattern == "endT":
            m[Tn] = False                      # the episode ends exactly at t + 1 == T
        elif pattern == "borders" and Tn > 0:
            m[cdiv(Tn, 64)::cdiv(Tn, 64)] = False    # an end on every border between two lanes' chunks of the scan
    m[0] = g.random(N) > 0.5                   # masks[0] is never read
    return NS(r=r, v=v, m=m.astype(np.uint8), nv=g.standard_normal(N).astype(f32))


def gae_ref(d, Tn, N, use_gae, scan=False, *, gamma=GAMMA, tau=TAU, round_hp=True, mask_on_trace=True, boot_from_entry=False):
    """float64 returns with their allowance, and value_preds after the call.
    k per step, use_gae: gamma * v' 1, + r 1, - v 1, gamma * tau as float 1, (gamma tau) * gae 1, + 1 = 6 (the mask multiplies are exact),
    and 1 for gae + v.  The scan composes each lane's chunk into a map (a, b) first: one more rounding per step in the product a and
    one where the map meets its neighbour = 8 per step, and the carry a lane receives went through 6 shuffle rounds of a multiply and
    an add each = 12 at the carry's magnitude, added at every chunk border.  The bound follows the recurrence itself:
    E_t = k OP (|r| + gamma |v'| m + |v| + c M_{t+1}) + c E_{t+1}, with M the same recurrence on absolute values.
    use_gae 0: gamma * R' 1, + r 1 = 2 per step, same recurrence."""
    gm, ta = (w32(gamma), w32(tau)) if round_hp else (gamma, tau)
    gt = gm * ta
    r, v, m = d.r.astype(f64), d.v.astype(f64).copy(), (d.m != 0).astype(f64)
    nv = d.nv.astype(f64)
    ret, err = np.full((Tn + 1, N), NAN), np.full((Tn + 1, N), NAN)
    k = 8 if scan else 6
    per = max(cdiv(Tn, 64), 1)
    if use_gae:
        if not boot_from_entry:
            v[Tn] = nv
        gae, M, E = np.zeros(N), np.zeros(N), np.zeros(N)
        for t in reversed(range(Tn)):
            c = gt * m[t + 1] if mask_on_trace else gt * np.ones(N)
            loc = np.abs(r[t]) + gm * np.abs(v[t + 1]) * m[t + 1] + np.abs(v[t])
            if scan and (t + 1) % per == 0 and t + 1 < Tn:
                E = E + 12 * OP * M
            E = k * OP * (loc + c * M) + c * E
            gae = r[t] + gm * v[t + 1] * m[t + 1] - v[t] + c * gae
            M = loc + c * M
            ret[t], err[t] = gae + v[t], E + OP * (M + np.abs(v[t]))
    else:
        ret[Tn], err[Tn] = nv, 0.0
        Rn, M, E = nv.copy(), np.abs(nv), np.zeros(N)
        for t in reversed(range(Tn)):
            c = gm * m[t + 1]
            E = 2 * OP * (c * M + np.abs(r[t])) + c * E
            Rn, M = c * Rn + r[t], c * M + np.abs(r[t])
            ret[t], err[t] = Rn, E
    return R(ret, np.nan_to_num(err, nan=0.0)), v


@functools.lru_cache(maxsize=None)
def gae_oracle(Tn, N, pattern, use_gae):
    """The float32 CPU loop of oracle.functional (what variant 0 must equal bit for bit)."""
    d = gae_data(Tn, N, pattern)
    sh = (Tn + 1, N, 1)
    ret, vp = O.compute_returns(T(d.r).view(sh), T(d.v).view(sh), T(d.m).view(sh), T(d.nv).view(N, 1), Tn, bool(use_gae), GAMMA, TAU)
    return ret.view(Tn + 1, N), vp.view(Tn + 1, N)


def gae_written(Tn, N, use_gae):
    wr, wv = np.zeros((Tn + 1, N), bool), np.zeros((Tn + 1, N), bool)
    if use_gae:
        wr[:Tn], wv[Tn] = True, True      # returns[T] is left alone, value_preds[T] = next_value
    else:
        wr[:] = True
    return wr, wv


@pytest.mark.parametrize("Tn,N", GAE_SHAPES)
def test_compute_returns_float32_loop_within_half(Tn, N):
    for pattern in PATTERNS:
        d = gae_data(Tn, N, pattern)
        for use_gae in (0, 1):
            ret, _ = gae_oracle(Tn, N, pattern, use_gae)
            wr, _ = gae_written(Tn, N, use_gae)
            got = np.where(wr, ret.numpy(), NAN)
            half("compute_returns", got, gae_ref(d, Tn, N, use_gae, scan=False)[0])


@gpu
@pytest.mark.parametrize("Tn,N", GAE_SHAPES)
def test_compute_returns(L, Tn, N):
    for pattern in PATTERNS:
        d = gae_data(Tn, N, pattern)
        for use_gae in (0, 1):
            wr, wv = gae_written(Tn, N, use_gae)
            oret, ovp = gae_oracle(Tn, N, pattern, use_gae)
            for variant in (0, 1):
                v0, r0 = guard(d.v), guard(nans((Tn + 1) * N))

                def run():
                    r, m, nv, v, ret = dev(d.r), dev(d.m), dev(d.nv), v0.cuda(), r0.cuda()
                    rc = L.hab_compute_returns(P(r), PB(v), P(m), PB(ret), P(nv), Tn, N, GAMMA, TAU, use_gae, variant, S())
                    torch.cuda.synchronize()
                    assert rc == 0
                    return dict(v=v.cpu(), ret=ret.cpu())
                o = twice(run)
                tag = f"T={Tn} N={N} {pattern} gae={use_gae} variant={variant}"
                assert untouched(r0, o["ret"], wr), tag + ": returns written where they must not be"
                assert untouched(v0, o["v"], wv), tag + ": value_preds written where they must not be"
                if use_gae:
                    assert same_bits(body(o["v"]).view(Tn + 1, N)[Tn], T(d.nv)), tag
                got = body(o["ret"]).view(Tn + 1, N)
                scan = bool(variant == 1 and use_gae and Tn > 0)
                if not scan:
                    assert same_bits(got[T(wr)], oret[T(wr)]), tag + ": not the bits of the float32 CPU loop"
                hold("hab_compute_returns " + ("scan" if scan else "exact"), got, gae_ref(d, Tn, N, use_gae, scan=scan)[0])


def test_compute_returns_wrong_variants_are_caught():
    for (Tn, N) in ((65, 3), (200, 65)):
        d = gae_data(Tn, N, "rand")
        ref, _ = gae_ref(d, Tn, N, 1, scan=True)
        assert caught(gae_ref(d, Tn, N, 1, mask_on_trace=False)[0], ref), "gamma * tau applied without the mask"
        assert caught(gae_ref(d, Tn, N, 1, boot_from_entry=True)[0], ref), "bootstrap from value_preds[T] as it was on entry"


# ================================================================================================
# hab_advantages
# ================================================================================================
ADV_COUNTS = (2, 63, 64, 65, 1023, 1024, 1025, 129 * 64)
EPS_ADV = w32(1e-5)


@functools.lru_cache(maxsize=None)
def adv_data(count, kind):
    g = rng(2, count, _key(kind))
    ret = (50.0 + g.standard_normal(count)).astype(f32)      # mean far from zero: a one-pass or float32 variance fails here
    val = (0.5 * g.standard_normal(count)).astype(f32)
    if kind == "holes":                                      # ~2 % NaN and a few infinities among the returns
        assert count >= 63
        ret[g.random(count) < 0.02] = NAN
        p = g.permutation(count)
        ret[p[0]], ret[p[1]], ret[p[2]] = NAN, np.inf, -np.inf
        ret[p[3:9]] = (50.0 + g.standard_normal(6)).astype(f32)     # at least two finite entries
    elif kind == "allbad":
        ret[:] = np.array([NAN, np.inf, -np.inf], f32)[g.integers(0, 3, count)]
    return NS(ret=ret, val=val, count=count)


def adv_ref(d, mode, ext=None, *, biased=False, local_mean=False, count_all=False):
    """raw: the float32 difference (exact: one _rn op).  Statistics and the normalised advantages in float64.
    k: adv 1; the mean and the sums of squares are formed in double from the rounded adv (they inherit its error, no rounding of their
    own); mean -> float 1, var -> float 1, + 1e-5 1, rsqrtf 2 ulp = 4, adv - mean 1, * rstd 1."""
    with np.errstate(all="ignore"):
        raw = d.ret - d.val
        a = sub(d.ret.astype(f64), d.val.astype(f64))
        fin = np.ones(d.count, bool) if count_all else np.isfinite(raw)
        Cn = float(fin.sum())
        out = NS(raw=raw, stats={}, adv=None)
        if mode == 0:
            return out
        ext = None if ext is None else np.asarray(ext, f32)
        local = R(a.v[fin].sum() / Cn, a.e[fin].sum() / Cn) if Cn > 0 else R(0.0)
        mean = local if mode in (1, 2) else rnd(local.v, local.e) if local_mean else R(f64(ext[0]))
        if mode == 2:
            out.stats = {0: rnd(mean.v, mean.e), 2: R(Cn)}
            return out
        if mode == 3:
            var = R(f64(ext[1]))
        else:
            dd = a.v[fin] - mean.v
            den = max(Cn, 1.0) if (mode == 4 or biased) else max(Cn - 1.0, 1.0)
            var = R((dd * dd).sum() / den, 2.0 * (np.abs(dd) * (a.e[fin] + mean.e)).sum() / den)
            if mode == 4:
                out.stats = {1: rnd(var.v, var.e), 2: R(Cn)}
                return out
            out.stats = {0: rnd(mean.v, mean.e), 1: rnd(var.v, var.e), 2: R(Cn)}
        rstd = rsqrt_(add(rnd(var.v, var.e), EPS_ADV), ulps=2)
        out.adv = mul(sub(a, rnd(mean.v, mean.e)), rstd)
        return out


def adv_f32(d, mode, ext=None):
    """float32 on the CPU in torch, the oracle's operations (get_advantages; its distributed form for modes 2 - 4)."""
    adv = T(d.ret) - T(d.val)
    fin = adv[torch.isfinite(adv)]
    if mode in (1, 2):
        var, mean = torch.var_mean(fin) if fin.numel() > 1 else (torch.zeros(()), fin.sum())
    if mode == 2:
        return None, {0: mean}
    if mode == 4:
        return None, {1: (fin - ext[0]).pow(2).mean()}
    if mode == 3:
        mean, var = ext[0], ext[1]
    return (adv - mean) * torch.rsqrt(var + O.EPS_PPO), ({0: mean, 1: var} if mode == 1 else {})


def adv_ext(d):
    """External statistics for the stand-alone mode 3 / mode 4 cases: deliberately not the local ones."""
    return torch.tensor([50.3, 1.7, 0.0])


def adv_cases():
    for count in ADV_COUNTS:
        yield count, "finite"
        if count >= 63:
            yield count, "holes"
    yield 65, "allbad"
    yield 1025, "allbad"


@pytest.mark.parametrize("count,kind", list(adv_cases()))
def test_advantages_float32_within_half(count, kind):
    if kind == "allbad":
        return  # nothing finite to evaluate; the GPU test pins what the kernel does
    d = adv_data(count, kind)
    for mode, ext in ((1, None), (2, None), (3, adv_ext(d)), (4, adv_ext(d))):
        ref = adv_ref(d, mode, ext)
        got, st = adv_f32(d, mode, ext)
        if ref.adv is not None:
            half(f"advantages mode {mode}", got, ref.adv)
        for i, x in st.items():
            half(f"advantages stats[{i}] mode {mode}", x, ref.stats[i])


ADV_WRITES = {0: (), 1: (0, 1, 2), 2: (0, 2), 3: (), 4: (1, 2)}


def adv_run(L, d, mode, ext=None, stats0=None, stats=True, alias=False):
    a0 = guard(nans(d.count))
    s0 = guard(nans(3) if stats0 is None else stats0)

    def run():
        ret, val, adv, st = dev(d.ret), dev(d.val), a0.cuda(), s0.cuda()
        e = PB(st) if alias else (P(dev(ext)) if ext is not None else None)
        rc = L.hab_advantages(P(ret), P(val), PB(adv), d.count, mode, e, PB(st) if stats else None, S())
        torch.cuda.synchronize()
        assert rc == 0
        return dict(adv=adv.cpu(), st=st.cpu())
    o = twice(run)
    assert untouched(a0, o["adv"], np.ones(d.count, bool)), f"mode {mode}: guard of adv"
    wr = np.zeros(3, bool)
    if stats:
        wr[list(ADV_WRITES[mode])] = True
    assert untouched(s0, o["st"], wr), f"mode {mode}: stats written where they must not be"
    return body(o["adv"]), body(o["st"])


def adv_check(name, d, mode, adv, st, ref, stats=True):
    if ref.adv is None:
        assert same_f32(adv, ref.raw), f"{name}: raw advantages are not the float32 difference"
    else:
        assert torch.equal(torch.isfinite(adv), T(np.isfinite(ref.raw))), f"{name}: non-finite entries must stay non-finite"
        hold("hab_advantages adv", adv, ref.adv)
    if stats:
        for i in ADV_WRITES[mode]:
            hold(f"hab_advantages stats[{i}]", st[i:i + 1], ref.stats[i])


@gpu
@pytest.mark.parametrize("count,kind", list(adv_cases()))
def test_advantages(L, count, kind):
    d = adv_data(count, kind)
    ext = adv_ext(d)
    for mode in range(5):
        e = ext if mode in (3, 4) else None
        adv, st = adv_run(L, d, mode, e, stats=mode in (1, 2, 4))
        adv_check(f"mode {mode}", d, mode, adv, st, adv_ref(d, mode, e), stats=mode in (1, 2, 4))
        if mode == 1:
            adv2, _ = adv_run(L, d, 1, None, stats=False)           # stats_out = NULL is legal
            assert same_bits(adv, adv2), "mode 1 without stats_out gives other advantages"
    # distributed_var_mean as ppo.py runs it in one process: 2 -> 4 -> 3 on ONE stats buffer that is ext_stats and stats_out at once
    _, st2 = adv_run(L, d, 2)
    r2 = adv_ref(d, 2)
    adv_check("2 of 2-4-3", d, 2, _, st2, r2)
    _, st4 = adv_run(L, d, 4, stats0=st2, alias=True)
    assert same_bits(st4[0:1], st2[0:1])
    adv_check("4 of 2-4-3", d, 4, _, st4, adv_ref(d, 4, None, local_mean=True))
    adv3, st3 = adv_run(L, d, 3, stats0=st4, alias=True, stats=False)
    assert same_bits(st3, st4)
    full = adv_ref(d, 1, None, biased=True)     # the three phases together: normalise by the biased variance about the mean
    assert torch.equal(torch.isfinite(adv3), T(np.isfinite(full.raw)))
    hold("hab_advantages adv 2-4-3", adv3, full.adv)
    if kind == "allbad":                        # pinned: nothing finite gives mean 0, var 0, count 0
        _, st1 = adv_run(L, d, 1)
        assert st1.tolist() == [0.0, 0.0, 0.0]


def test_advantages_wrong_variants_are_caught():
    for count in (65, 129 * 64):
        d = adv_data(count, "finite")
        ref = adv_ref(d, 1)
        b = adv_ref(d, 1, biased=True)
        assert caught(b.adv, ref.adv) and caught(b.stats[1], ref.stats[1]), "biased instead of unbiased variance in mode 1"
        ext = adv_ext(d)
        assert caught(adv_ref(d, 4, ext, local_mean=True).stats[1], adv_ref(d, 4, ext).stats[1]), "mode 4 about the local mean"
    for count in (65, 1025):
        d = adv_data(count, "holes")
        for mode in (1, 2):
            ref, bad = adv_ref(d, mode), adv_ref(d, mode, count_all=True)
            assert caught(bad.stats[0], ref.stats[0]) and caught(bad.stats[2], ref.stats[2]), "statistics that count non-finite entries"
        assert caught(adv_ref(d, 1, count_all=True).adv, adv_ref(d, 1).adv)
    # and the reason for the double-precision two-pass form: a float32 one-pass variance misses the bar at this mean
    d = adv_data(129 * 64, "finite")
    a = T(d.ret) - T(d.val)
    one_pass = (a * a).mean() - a.mean() ** 2
    assert caught(one_pass.numpy() * d.count / (d.count - 1), adv_ref(d, 1).stats[1])


# ================================================================================================
# hab_ppo_loss / hab_ppo_loss_ver
# ================================================================================================
LOSS_B = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
VCOEF, ECOEF, THRESH, LOG_ALPHA, CUR_VERSION = 0.5, 0.01, 0.7, -1.25, 1000
N_PLANTS = 10


@functools.lru_cache(maxsize=None)
def loss_data(B, rows, clip):
    g = rng(3, B, int(rows), int(clip * 100))
    Gs = B + 37 if rows else B
    idx = g.permutation(Gs)[:B] if rows else np.arange(B)
    olp = (-(np.abs(g.standard_normal(B)) + 0.1)).astype(f32)
    lp = (olp + 0.15 * g.standard_normal(B)).astype(f32)
    a = g.standard_normal(B).astype(f32)
    ov = g.standard_normal(B).astype(f32)
    v = (ov + 0.2 * g.standard_normal(B)).astype(f32)
    ret = (ov + 0.5 * g.standard_normal(B)).astype(f32)
    en = (1.4 * g.random(B)).astype(f32)
    c32 = f32(clip)
    c = float(c32)
    ov0 = f32(0.5) if clip == 0.25 else f32(0.0)    # 0.5 +- 0.25 is exact; 0.2f is only exact against 0
    fixed_v = np.zeros(B, bool)

    def plant(k, p):
        if k == 0:      # adv = 0, ratio far from 1
            a[p], lp[p] = 0.0, f32(olp[p] + f32(0.5))
        elif k == 1:    # logp bitwise old_logp: ratio exactly 1, s1 == s2, gradient weight 1
            lp[p] = olp[p]
        elif k == 2:    # adv = 0 and ratio 1
            a[p], lp[p] = 0.0, olp[p]
        elif k in (3, 4, 5, 6):   # ratio far outside the clip range, each sign of adv: the four cases of min with clamp
            lp[p] = f32(olp[p] + f32(1.0 if k < 5 else -1.0))
            a[p] = 1.5 if k in (3, 5) else -1.5
        elif k in (7, 8):         # v - old_v == +-clip exactly: `<` is strict, so the clipped branch, d_value = 0
            ov[p], v[p], fixed_v[p] = ov0, (ov0 + c32 if k == 7 else ov0 - c32), True
        else:                     # just inside the clip
            ov[p], v[p], fixed_v[p] = 0.0, np.nextafter(c32, f32(0.0)), True
    low = min(B, 1024)
    if low >= 5 * N_PLANTS:
        for k in range(N_PLANTS):
            plant(k, 5 * k + 2)
    else:
        plant(B % N_PLANTS, 0)
    if B >= 1024 + 5 * N_PLANTS:
        for k in range(N_PLANTS):
            plant(k, 1024 + 5 * k + 2)
    elif B > 1024:
        plant(7, 1024)
    # no float64 ratio within 1e-4 relative of 1 +- clip, no |v - old_v| within 1e-4 relative of clip (planted frames apart): a draw
    # that is moves on, so every branch the kernel takes in float32 is the branch the reference takes
    for _ in range(100):
        rr = np.exp(lp.astype(f64) - olp.astype(f64))
        bad = (np.abs(rr / (1.0 - c) - 1.0) < 1e-4) | (np.abs(rr / (1.0 + c) - 1.0) < 1e-4)
        dl = np.abs(v.astype(f64) - ov.astype(f64))
        badv = (np.abs(dl / c - 1.0) < 1e-4) & ~fixed_v
        if not bad.any() and not badv.any():
            break
        lp[bad] = (lp[bad] + f32(0.01)).astype(f32)
        v[badv] = (v[badv] + f32(0.01)).astype(f32)
    else:
        raise AssertionError("could not move the draws off the clip edges")
    isc = (0.3 + 1.4 * g.random(B)).astype(f32)
    isc[g.random(B) < 0.3] = 1.0
    pick = g.permutation(B)[:min(B, 4)]
    isc[pick] = np.array([40.0, 1.0, 0.25, 7.5], f32)[:len(pick)]
    stale = (g.random(B) < 0.3).astype(np.uint8)
    pv = (CUR_VERSION - g.integers(0, 50, B)).astype(np.int64)

    def store(x, fill):
        s = np.full(Gs, fill, x.dtype)
        s[idx] = x
        return s
    return NS(B=B, idx=idx, rows=idx.astype(np.int32) if rows else None, v=v, lp=lp, en=en, olp=olp, a=a, ov=ov, ret=ret, isc=isc,
              stale=stale, pv=pv, clip=clip,
              S=NS(olp=store(olp, NAN), a=store(a, NAN), ov=store(ov, NAN), ret=store(ret, NAN), isc=store(isc, NAN),
                   stale=store(stale, 1), pv=store(pv, -10 ** 12)))


def loss_ref(d, clip_value, use=(), log_alpha=None, *, le=False, maxform=False, tie_weight=0.5, clamp_is=True, by_sum_w=False):
    """use: which of "isc", "stale", "pv" are given.  Returns dv, dlp, den (R [B]) and out (R [24], NaN where nothing is written).
    k, per frame: ratio = expf(logp - old) 1 + 2 ulp (4) = 5; lo / hi = 1 -+ clip 1; s = adv * ratio 1; weights wf 1 each; 1/B 1 and the
    multiply by it 1.  d_logp 5 + 4 = 9; d_value v - ret 1 + 4 multiplies/1/B = 5; d_entropy 3 (+ 4 for expf(log_alpha)).  Means: the
    per-frame bound summed, + (cdiv(B, 1024) + 21) OP sum |term| for the adds on the longest path (cdiv(B, 1024) - 1 in the thread, 6
    shuffle rounds, 16 partials), + 2 for 1/B.  Minima and maxima of inputs, counts and B are exact."""
    B, c = d.B, w32(d.clip)
    one = lambda x: R(x.astype(f64))
    v, lp, en, olp, a, ov, ret = one(d.v), one(d.lp), one(d.en), one(d.olp), one(d.a), one(d.ov), one(d.ret)
    lo, hi = rnd(1.0 - c), rnd(1.0 + c)
    ratio = exp_(sub(lp, olp), ulps=2)
    rc = min_(max_(ratio, lo), hi)
    s1, s2 = mul(a, ratio), mul(a, rc)
    al = neg(min_(s1, s2))
    isc = one(d.isc) if "isc" in use else R(np.ones(B))
    wf = min_(isc, 1.0) if clamp_is else isc
    inr = (ratio.v >= lo.v) & (ratio.v <= hi.v)
    w = np.where(s1.v < s2.v, 1.0, np.where(s1.v == s2.v, np.where(inr, 1.0, tie_weight), inr.astype(f64)))
    invB = rnd(1.0 / B)
    dlp = mul(mul(mul(mul(neg(a), w, k=0), ratio), invB), wf)
    if clip_value:
        delta = sub(v, ov)
        keep = (np.abs(delta.v) <= c) if le else (np.abs(delta.v) < c)
        clipped = add(ov, R(np.clip(delta.v, -c, c), delta.e))
        vv = where_(keep, v, clipped)
        dv = where_(keep, sub(v, ret), 0.0)
        e = sub(vv, ret)
        vl = mul(0.5, mul(e, e), k=0)
        if maxform:      # 0.5 max((v - ret)^2, (clipped - ret)^2), the other common form
            e1, e2 = sub(v, ret), sub(clipped, ret)
            first = e1.v * e1.v >= e2.v * e2.v
            vl = mul(0.5, where_(first, mul(e1, e1), mul(e2, e2)), k=0)
            dv = where_(first, e1, where_(keep, e2, 0.0))
    else:
        dv = sub(v, ret)
        vl = mul(0.5, mul(dv, dv), k=0)
    vc = R(w32(VCOEF))
    ec = exp_(R(f64(f32(log_alpha))), ulps=2) if log_alpha is not None else R(w32(ECOEF))
    dvo = mul(mul(mul(vc, dv), invB), wf)
    den = mul(mul(neg(ec), invB), wf)
    den = R(np.broadcast_to(den.v, (B,)).copy(), np.broadcast_to(den.e, (B,)).copy())
    depth = cdiv(B, 1024) + 21
    i32B = f32(1.0) / f32(B)

    def mean_(t):
        s = R(t.v.sum(), t.e.sum() + depth * OP * np.abs(t.v).sum())
        return div(s, wf.v.sum(), k=2) if by_sum_w else mul(s, invB)

    def count_(n):       # an exact float32 count times the float32 1/B: exact in the reference too
        return R(f64(f32(n) * i32B))
    vlm, alm, enm = mean_(mul(wf, vl)), mean_(mul(wf, al)), mean_(mul(wf, en))
    out = [R(NAN)] * 24
    out[0], out[1], out[2] = vlm, alm, enm
    if log_alpha is None:
        out[3] = sub(add(mul(vc, vlm), alm), mul(ec, enm))
    else:
        t1 = mul(ec, sub(w32(THRESH), enm))
        out[3] = add(add(mul(vc, vlm), alm), sub(t1, mul(ec, enm)))
        out[20], out[21] = t1, ec
    out[4], out[5], out[6] = R(v.v.min()), mean_(v), R(v.v.max())
    out[7], out[8], out[9] = R(ratio.v.min(), ratio.e.max()), mean_(ratio), R(ratio.v.max(), ratio.e.max())
    out[10] = count_(((ratio.v > hi.v) | (ratio.v < lo.v)).sum())
    out[11] = R(float(B))
    if use:
        if "isc" in use:
            out[13], out[14], out[15] = R(isc.v.min()), mean_(isc), R(isc.v.max())
        else:            # pinned: the empty minimum, mean and maximum the kernel writes for an input that is not given
            out[13], out[14], out[15] = R(np.inf), R(0.0), R(-np.inf)
        out[16] = count_(d.stale.sum()) if "stale" in use else R(0.0)
        if "pv" in use:
            dd = (CUR_VERSION - d.pv).astype(f64)
            out[17], out[18], out[19] = R(dd.min()), count_(dd.sum()), R(dd.max())
        else:
            out[17], out[18], out[19] = R(np.inf), R(0.0), R(-np.inf)
    return NS(dv=dvo, dlp=dlp, den=den, out=R(np.array([o.v for o in out]), np.array([float(o.e) for o in out])))


def loss_f32(d, clip_value, use=(), log_alpha=None):
    """oracle.functional.ppo_loss in float32 with autograd for the three gradients, and the metrics in plain torch."""
    v, lp, en = (T(x).clone().requires_grad_(True) for x in (d.v, d.lp, d.en))
    batch = dict(action_log_probs=T(d.olp), advantages=T(d.a), value_preds=T(d.ov), returns=T(d.ret))
    if "isc" in use:
        batch["is_coeffs"] = T(d.isc)
    ec = ECOEF
    if log_alpha is not None:
        la = torch.tensor(log_alpha, requires_grad=True)
        ec = dict(log_alpha=la, threshold=THRESH)
    total, vl, al, ent, ratio = O.ppo_loss(v, lp, en, batch, d.clip, VCOEF, ec, bool(clip_value))
    total.backward()
    out = torch.full((24,), NAN)
    out[0], out[1], out[2], out[3] = vl.detach(), al.detach(), ent.detach(), total.detach()
    out[4], out[5], out[6] = v.min().detach(), v.mean().detach(), v.max().detach()
    r = ratio.detach()
    out[7], out[8], out[9] = r.min(), r.mean(), r.max()
    out[10] = ((r > 1.0 + d.clip) | (r < 1.0 - d.clip)).float().mean()
    out[11] = d.B
    if log_alpha is not None:
        out[20], out[21] = la.grad, torch.exp(la.detach())
    if use:
        if "isc" in use:
            out[13], out[14], out[15] = T(d.isc).min(), T(d.isc).mean(), T(d.isc).max()
        else:
            out[13], out[14], out[15] = math.inf, 0.0, -math.inf
        out[16] = T(d.stale).float().mean() if "stale" in use else 0.0
        if "pv" in use:
            dd = (CUR_VERSION - T(d.pv)).float()
            out[17], out[18], out[19] = dd.min(), dd.mean(), dd.max()
        else:
            out[17], out[18], out[19] = math.inf, 0.0, -math.inf
    return v.grad, lp.grad, en.grad, out


OUT_GROUP = {i: g for g, idx in (("0..3 losses", (0, 1, 2, 3)), ("4..9 value and ratio", (4, 5, 6, 7, 8, 9)), ("10 11 counts", (10, 11)),
                                 ("13..19 VER", range(13, 20)), ("20 21 alpha", (20, 21))) for i in idx}
VER_USES = ((("isc", "stale", "pv"), True), (("stale", "pv"), False), (("isc", "pv"), True), (("isc", "stale"), False), ((), True))


def loss_cases(B):
    """(rows, clip, clip_value, use, log_alpha, through the _ver entry point)."""
    for rows in (False, True):
        for clip in (0.2, 0.25):
            for cv in (0, 1):
                yield rows, clip, cv, (), None, False
    for i, (use, la) in enumerate(VER_USES):
        yield bool(i % 2), (0.2, 0.25)[(i // 2) % 2], 1 - i % 2, use, (LOG_ALPHA if la else None), True
    yield True, 0.25, 1, (), None, True      # nothing of VER given and no log_alpha: out[12..] stays NaN


@pytest.mark.parametrize("B", LOSS_B)
def test_ppo_loss_float32_within_half(B):
    for rows, clip, cv, use, la, _ in loss_cases(B):
        if rows:
            continue     # the same frames in another storage order
        d = loss_data(B, rows, clip)
        ref = loss_ref(d, cv, use, la)
        dv, dlp, den, out = loss_f32(d, cv, use, la)
        half("ppo_loss d_value", dv, ref.dv)
        half("ppo_loss d_logp", dlp, ref.dlp)
        half("ppo_loss d_entropy", den, ref.den)
        exact = [i for i in range(24) if i not in (10, 16, 18)]     # the oracle forms these three as means, not as count / B
        half("ppo_loss out", out.numpy()[exact], ref.out[exact])
        for i in (10, 16, 18):
            if not np.isnan(ref.out.v[i]):
                assert abs(float(out[i]) - ref.out.v[i]) <= 4 * U * abs(ref.out.v[i]) * (cdiv(B, 1024) + 21)


@gpu
@pytest.mark.parametrize("B", LOSS_B)
def test_ppo_loss(L, B):
    for rows, clip, cv, use, la, ver in loss_cases(B):
        d = loss_data(B, rows, clip)
        ref = loss_ref(d, cv, use, la)
        g0, o0 = guard(nans(B)), guard(nans(24))

        def run():
            ins = [dev(x) for x in (d.v, d.lp, d.en, d.S.olp, d.S.a, d.S.ov, d.S.ret)]
            rw = dev(d.rows) if rows else None
            dv, dlp, den, out = g0.cuda(), g0.cuda(), g0.cuda(), o0.cuda()
            head = [P(x) for x in ins] + [P(rw), B, clip, VCOEF, ECOEF, cv]
            tail = [PB(dv), PB(dlp), PB(den), PB(out), S()]
            if ver:
                isc = dev(d.S.isc) if "isc" in use else None
                st = dev(d.S.stale) if "stale" in use else None
                pv = dev(d.S.pv) if "pv" in use else None
                lat = torch.tensor([la], dtype=torch.float32).cuda() if la is not None else None
                rc = L.hab_ppo_loss_ver(*head, P(isc), P(st), P(pv), CUR_VERSION, P(lat), THRESH, *tail)
            else:
                rc = L.hab_ppo_loss(*head, *tail)
            torch.cuda.synchronize()
            assert rc == 0
            return dict(dv=dv.cpu(), dlp=dlp.cpu(), den=den.cpu(), out=out.cpu())
        o = twice(run)
        tag = f"B={B} rows={rows} clip={clip} clip_value={cv} use={use} log_alpha={la}"
        for k in ("dv", "dlp", "den"):
            assert untouched(g0, o[k], np.ones(B, bool)), tag + f": guard of {k}"
        assert untouched(o0, o["out"], ~np.isnan(ref.out.v)), tag + ": out written where it must not be"
        ep = "hab_ppo_loss_ver" if ver else "hab_ppo_loss"
        hold(ep + " d_value", body(o["dv"]), ref.dv)
        hold(ep + " d_logp", body(o["dlp"]), ref.dlp)
        hold(ep + " d_entropy", body(o["den"]), ref.den)
        out = body(o["out"]).numpy()
        for i in range(24):      # minima, maxima, counts and B have allowance 0: they are held to ==
            if not np.isnan(ref.out.v[i]):
                hold(f"{ep} out[{OUT_GROUP[i]}]", out[i:i + 1], ref.out[i:i + 1])


def test_ppo_loss_wrong_variants_are_caught():
    for B in (65, 2500):
        for clip in (0.2, 0.25):
            d = loss_data(B, False, clip)
            ref = loss_ref(d, 1, ("isc", "stale", "pv"), LOG_ALPHA)
            bad = loss_ref(d, 1, ("isc", "stale", "pv"), LOG_ALPHA, le=True)
            assert caught(bad.dv, ref.dv), "<= instead of < in the value clip"
            bad = loss_ref(d, 1, ("isc", "stale", "pv"), LOG_ALPHA, maxform=True)
            assert caught(bad.dv, ref.dv) and caught(bad.out[0:1], ref.out[0:1]), "max-of-two-losses form of the clipped value loss"
            bad = loss_ref(d, 1, ("isc", "stale", "pv"), LOG_ALPHA, clamp_is=False)
            assert caught(bad.dlp, ref.dlp) and caught(bad.out[1:2], ref.out[1:2]), "is_coeffs not clamped at 1"
            bad = loss_ref(d, 1, ("isc", "stale", "pv"), LOG_ALPHA, by_sum_w=True)
            for i in (0, 1, 2, 3, 20):
                assert caught(bad.out[i:i + 1], ref.out[i:i + 1]), f"means divided by the sum of the weights: out[{i}]"


def test_tie_weight_is_unobservable():
    """The listed variant `tie weight 1 where 0.5 is due` cannot exceed any allowance: s1 == s2 with the ratio outside [lo, hi] needs
    adv == 0 (adv * ratio == adv * clamp(ratio) with ratio != clamp(ratio)), and d_logp = -adv * w * ratio / B is then 0 for every w.
    Pinned here on the planted adv == 0 frames, so that a change of the inputs which makes the weight observable shows up."""
    for B in (65, 2500):
        d = loss_data(B, False, 0.25)
        ref, one, zero = loss_ref(d, 1), loss_ref(d, 1, tie_weight=1.0), loss_ref(d, 1, tie_weight=0.0)
        ties = (d.a == 0) & (d.lp != d.olp)
        assert ties.sum() >= 1
        assert np.array_equal(ref.dlp.v, one.dlp.v) and np.array_equal(ref.dlp.v, zero.dlp.v)
        assert (ref.dlp.v[ties] == 0).all() and (ref.dlp.e[ties] == 0).all()


# ================================================================================================
# hab_clip_adam_step
# ================================================================================================
LR, B1, B2, EPS = 2.5e-4, 0.9, 0.999, 1e-5
N3 = 4 * 256 * 3 + 2
N1K = 4 * 256 * 1024 + 7     # one float4 block more than the 1024-block cap of the norm pass
N2K = 4 * 256 * 2048 + 5     # ... than the 2048-block cap of the update pass
SCRATCH = 4096
# (n, scratch_len, max-norm as a factor of the true norm (0 and < 0: no clipping), grad_scale, step, kind)
ADAM_CASES = (
    [(n, (1, 7, 1024, 4096)[i % 4], (0.1, 10.0, 0.0, -1.0)[i % 4], (1.0, 0.5)[i % 2], 1, "cold")
     for i, n in enumerate((1, 3, 4, 5, 1023, 1025, N3))]
    + [(N3, sl, 0.1, 0.5, 1, "cold") for sl in (1, 7, 1024, 4096)]
    + [(N3, 1024, f, 1.0, 1, "cold") for f in (0.1, 10.0, 0.0, -1.0)]
    + [(N1K, 4096, 0.1, 0.5, 1, "cold"), (N1K, 7, 10.0, 1.0, 2, "warm"), (N2K, 1024, 0.1, 1.0, 1, "cold"), (N2K, 1, -1.0, 0.5, 3, "warm")]
    + [(1025, 1024, 0.1, 1.0, s, "seq") for s in (1, 2, 3)]
    + [(1025, 1024, 0.1, 0.5, 100000, "warm"), (5, 1024, 0.1, 1.0, 1, "zero"), (N3, 7, 0.0, 1.0, 1, "zero"), (1023, 1024, 0.1, 1.0, 1, "tiny")]
)
ADAM_SMALL = [c for c in ADAM_CASES if c[0] <= N3]


def adam_ref(d, *, bias_correction=True, clip_eps=True):
    """k: norm: g * scale 1, square 1 (sum and sqrt in double), -> float 1.  coefficient: norm + 1e-6 1, divide 1, * scale 1.  Per element:
    g * coef 1; exp_avg: g - m 1, w1 -> float 1, * 1, + 1; exp_avg_sq: v * beta2 1, g * g 1, w2 -> float 1, * 1, + 1; sqrtf 1,
    sqrt(bc2) -> float 1, / 1, + eps 1, m / denom 1, lr / bc1 -> float 1, * 1, p - 1."""
    gs, mg = R(w32(d.gs)), w32(d.mgn)
    b1, b2 = w32(B1), w32(B2)
    g = R(d.g.astype(f64))
    sq = mul(mul(g, gs), mul(g, gs))
    norm = sqrt_(R(sq.v.sum(), sq.e.sum()), k=1)
    if mg > 0:
        coef = mul(min_(div(mg, add(norm, w32(1e-6)) if clip_eps else norm), 1.0), gs)
    else:
        coef = gs
    gg = mul(g, coef)
    m, v, p = R(d.m.astype(f64)), R(d.v.astype(f64)), R(d.p.astype(f64))
    m2 = add(m, mul(rnd(1.0 - b1), sub(gg, m)))
    v2 = add(mul(v, b2), mul(rnd(1.0 - b2), mul(gg, gg)))
    bc1, bc2 = (1.0 - b1 ** d.step, 1.0 - b2 ** d.step) if bias_correction else (1.0, 1.0)
    denom = add(div(sqrt_(v2), rnd(math.sqrt(bc2))), w32(EPS))
    p2 = sub(p, mul(rnd(w32(LR) / bc1), div(m2, denom)))
    return NS(p=p2, m=m2, v=v2, norm=norm)


@functools.lru_cache(maxsize=6)
def adam_data(n, factor, gs, step, kind):
    g_ = rng(4, n, int(factor * 10), int(gs * 10), step, _key(kind))
    if kind == "seq" and step > 1:      # the state after the previous step of the sequence: its reference rounded to float32
        prev = adam_data(n, factor, gs, step - 1, kind)
        r = adam_ref(prev)
        p, m, v = (x.v.astype(f32) for x in (r.p, r.m, r.v))
    else:
        p = g_.standard_normal(n).astype(f32)
        warm = kind == "warm"
        m = (0.01 * g_.standard_normal(n)).astype(f32) if warm else np.zeros(n, f32)
        v = (1e-4 * g_.random(n)).astype(f32) if warm else np.zeros(n, f32)
    scale = {"zero": 0.0, "tiny": 1e-4}.get(kind, 0.01)
    g = (scale * g_.standard_normal(n) * g_.random(n) ** 2).astype(f32)
    norm = math.sqrt(((g.astype(f64) * w32(gs)) ** 2).sum())
    mgn = factor * norm if factor > 0 and norm > 0 else (0.5 if factor > 0 else factor)
    return NS(n=n, p=p, g=g, m=m, v=v, gs=gs, mgn=w32(mgn), step=step)


def adam_f32(d):
    """oracle.functional's clip_grad_norm and adam_step (torch.optim.Adam's operations) in float32."""
    p, m, v = T(d.p).clone(), T(d.m).clone(), T(d.v).clone()
    g = T(d.g) * d.gs
    # the norm with its squares summed in double, as the kernel's partials are: torch's float32 accumulation is hundreds of allowances
    # off at n = 2^21, which is the reference's loss and no bar for the kernel
    norm = (g * g).double().sum().sqrt().float()
    if d.mgn > 0:
        g.mul_(torch.clamp(d.mgn / (norm + 1e-6), max=1.0))       # oracle.functional.clip_grad_norm's coefficient
    O.adam_step(p, g, m, v, d.step, w32(LR), w32(EPS), w32(B1), w32(B2))      # the hyper-parameters as the C ABI carries them
    return p, m, v, norm


@pytest.mark.parametrize("case", ADAM_CASES, ids=str)
def test_clip_adam_float32_within_half(case):
    n, sl, factor, gs, step, kind = case
    d = adam_data(n, factor, gs, step, kind)
    ref = adam_ref(d)
    p, m, v, norm = adam_f32(d)
    half("clip_adam params", p, ref.p)
    half("clip_adam exp_avg", m, ref.m)
    half("clip_adam exp_avg_sq", v, ref.v)
    half("clip_adam norm", norm, ref.norm)


@gpu
@pytest.mark.parametrize("case", ADAM_CASES, ids=str)
def test_clip_adam_step(L, case):
    n, sl, factor, gs, step, kind = case
    d = adam_data(n, factor, gs, step, kind)
    ref = adam_ref(d)
    p0, m0, v0, n0 = guard(d.p, -3.0), guard(d.m, -3.0), guard(d.v, -3.0), guard(nans(1))
    s0 = torch.full((SCRATCH,), NAN, dtype=torch.float64)

    def run():
        p, m, v, g, no, sc = p0.cuda(), m0.cuda(), v0.cuda(), guard(d.g, -3.0).cuda(), n0.cuda(), s0.cuda()
        rc = L.hab_clip_adam_step(PB(p), PB(g), PB(m), PB(v), n, P(sc), sl, gs, d.mgn, LR, B1, B2, EPS, step, PB(no), S())
        torch.cuda.synchronize()
        assert rc == 0
        return dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), no=no.cpu(), sc=sc.cpu(), g=g.cpu())
    o = twice(run)
    allw = np.ones(n, bool)
    for k, init in (("p", p0), ("m", m0), ("v", v0)):
        assert untouched(init, o[k], allw), f"{k}: the floats around n"
    assert same_bits(o["g"], guard(d.g, -3.0)), "the gradient is an input"
    assert untouched(n0, o["no"], np.ones(1, bool))
    used = min(sl, 1024)
    assert same_bits(o["sc"][used:], s0[used:]), "scratch written behind min(scratch_len, 1024)"
    hold("hab_clip_adam_step params", body(o["p"]), ref.p)
    hold("hab_clip_adam_step exp_avg", body(o["m"]), ref.m)
    hold("hab_clip_adam_step exp_avg_sq", body(o["v"]), ref.v)
    hold("hab_clip_adam_step grad_norm", body(o["no"]), ref.norm)
    if kind == "zero":
        assert same_bits(body(o["p"]), T(d.p)), "an all-zero gradient moved the parameters"


def test_clip_adam_wrong_variants_are_caught():
    d = adam_data(1025, 0.1, 1.0, 2, "seq")
    ref, bad = adam_ref(d), adam_ref(d, bias_correction=False)
    assert caught(bad.p, ref.p), "Adam without bias correction"
    d = adam_data(1023, 0.1, 1.0, 1, "tiny")
    ref, bad = adam_ref(d), adam_ref(d, clip_eps=False)
    assert caught(bad.m, ref.m) and caught(bad.v, ref.v), "a clip coefficient without the 1e-6"


# ================================================================================================
# hab_lagrange_adam_step
# ================================================================================================
LA_LR = 1e-3
LA_LO, LA_HI = math.log(1e-4), 0.0


def lagrange_ref(c, *, bias_correction=True):
    """k: grad * scale 1; exp_avg: g - m 1, 1 - b1 1, * 1, + 1; exp_avg_sq: v * b2 1, 1 - b2 1, two multiplies 2, + 1; powf 2 ulp (4) and
    1 - . 1 for each correction; sqrtf 1 each, / 1, + eps 1; lr / bc1 1, m / denom 1, * 1, log_alpha - . 1; expf 2 ulp (4)."""
    b1, b2 = w32(B1), w32(B2)
    g = mul(f64(c.grad), w32(c.gs))
    m, v = R(f64(c.m)), R(f64(c.v))
    m2 = add(m, mul(sub(g, m), rnd(1.0 - b1)))
    v2 = add(mul(v, b2), mul(mul(rnd(1.0 - b2), g), g))
    if bias_correction:
        bc1, bc2 = sub(1.0, rnd(b1 ** c.step, k=2)), sub(1.0, rnd(b2 ** c.step, k=2))
    else:
        bc1, bc2 = R(1.0), R(1.0)
    denom = add(div(sqrt_(v2), sqrt_(bc2)), w32(EPS))
    p = sub(f64(c.la), mul(div(w32(LA_LR), bc1), div(m2, denom)))
    lo, hi = w32(c.lo), w32(c.hi)
    assert not (abs(p.v - lo) <= p.e or abs(p.v - hi) <= p.e), "case too close to the projection's edge"
    pc = R(np.clip(p.v, lo, hi), np.where((p.v > lo) & (p.v < hi), p.e, 0.0))
    return NS(la=pc, m=m2, v=v2, alpha=exp_(pc, ulps=2))


def lagrange_cases():
    """Steps 1 - 5 from zero state with gradients of both signs (each step starts from the rounded reference of the one before), one at
    step 100000 from non-zero moments, grad_scale 0.5, and the two projections."""
    out = []
    st = NS(la=f32(-1.0), m=f32(0), v=f32(0))
    for step, grad in enumerate((0.7, -1.3, 0.2, -0.05, 2.0), 1):
        c = NS(la=st.la, m=st.m, v=st.v, grad=f32(grad), gs=(1.0, 0.5)[step % 2], step=step, lo=LA_LO, hi=LA_HI)
        out.append(c)
        r = lagrange_ref(c)
        st = NS(la=f32(r.la.v), m=f32(r.m.v), v=f32(r.v.v))
    out.append(NS(la=f32(-2.5), m=f32(0.03), v=f32(0.002), grad=f32(-0.4), gs=0.5, step=100000, lo=LA_LO, hi=LA_HI))
    out.append(NS(la=f32(-0.0002), m=f32(0), v=f32(0), grad=f32(-1.0), gs=1.0, step=1, lo=-0.5, hi=0.0))       # lands above max
    out.append(NS(la=f32(-0.4998), m=f32(0), v=f32(0), grad=f32(1.0), gs=1.0, step=1, lo=-0.5, hi=0.0))        # lands below min
    return out


def test_lagrange_float32_within_half():
    for c in lagrange_cases():
        ref = lagrange_ref(c)
        p, m, v = torch.tensor([c.la]), torch.tensor([c.m]), torch.tensor([c.v])
        O.adam_step(p, torch.tensor([c.grad]) * c.gs, m, v, c.step, w32(LA_LR), w32(EPS), w32(B1), w32(B2))
        p.clamp_(c.lo, c.hi)
        half("lagrange log_alpha", p, ref.la)
        half("lagrange exp_avg", m, ref.m)
        half("lagrange exp_avg_sq", v, ref.v)
        half("lagrange alpha", p.exp(), ref.alpha)
    c = lagrange_cases()[1]
    assert caught(lagrange_ref(c, bias_correction=False).la, lagrange_ref(c).la), "Adam without bias correction"
    hits = [lagrange_ref(c).la.v for c in lagrange_cases()[-2:]]
    assert hits[0] == 0.0 and hits[1] == -0.5, "the projection cases do not reach the bounds"


@gpu
def test_lagrange_adam_step(L):
    for c in lagrange_cases():
        ref = lagrange_ref(c)
        for with_alpha in (True, False):
            s0 = {k: guard(torch.tensor([x], dtype=torch.float32)) for k, x in (("la", c.la), ("m", c.m), ("v", c.v))}
            a0 = guard(nans(1))

            def run():
                la, m, v, al = s0["la"].cuda(), s0["m"].cuda(), s0["v"].cuda(), a0.cuda()
                g = torch.tensor([c.grad], dtype=torch.float32).cuda()
                rc = L.hab_lagrange_adam_step(PB(la), PB(m), PB(v), P(g), c.gs, LA_LR, B1, B2, EPS, c.step, c.lo, c.hi,
                                              PB(al) if with_alpha else None, S())
                torch.cuda.synchronize()
                assert rc == 0
                return dict(la=la.cpu(), m=m.cpu(), v=v.cpu(), al=al.cpu())
            o = twice(run)
            for k in ("la", "m", "v"):
                assert untouched(s0[k], o[k], np.ones(1, bool))
            assert untouched(a0, o["al"], np.ones(1, bool) if with_alpha else None)
            hold("hab_lagrange_adam_step log_alpha", body(o["la"]), ref.la)
            hold("hab_lagrange_adam_step exp_avg", body(o["m"]), ref.m)
            hold("hab_lagrange_adam_step exp_avg_sq", body(o["v"]), ref.v)
            if with_alpha:
                hold("hab_lagrange_adam_step alpha_out", body(o["al"]), ref.alpha)


# ================================================================================================
# hab_ver_compute_returns
# ================================================================================================
def _ver_spec(name):
    g = rng(5, _key(name))
    if name == "one":
        return [[9]]
    if name == "len1":
        return [[1], [1, 1, 1], [1], [1, 1]]
    envs, eps = {"F63": (9, 7), "F64": (8, 8), "F65": (13, 5), "F130": (13, 10)}[name]
    return [[int(x) for x in g.integers(1, 8, eps)] for _ in range(envs)]


VER_NAMES = ("one", "len1", "F63", "F64", "F65", "F130")
VER_PAD = 9


@functools.lru_cache(maxsize=None)
def ver_data(name):
    g = rng(6, _key(name))
    ep, env, step = [], [], []
    for e, lens in enumerate(_ver_spec(name)):
        t = 0
        for k, ln in enumerate(lens):
            for _ in range(ln):
                ep.append(k + 2 * e); env.append(e); step.append(t)
                t += 1
    n = len(ep)
    perm = g.permutation(n)                      # the steps sit in the buffer in no particular order
    ep, env, step = (np.array(x, np.int64)[perm] for x in (ep, env, step))
    info = pack_info_from_ids_np(ep, env, step)
    slots = np.sort(g.choice(n + VER_PAD, n, replace=False))   # ... and the buffer has slots that no sequence names
    sel = slots[info["select_inds"]]
    nseq = info["num_seqs_at_step"]
    offs = np.zeros(len(nseq) + 1, np.int64)
    offs[1:] = np.cumsum(nseq)
    lens, last = info["sequence_lengths"], info["last_sequence_in_batch_mask"]
    F = len(lens)
    nb = n + VER_PAD
    named = np.zeros(nb, bool)
    named[slots] = True
    rew, val, ret0 = np.full(nb, NAN, f32), np.full(nb, NAN, f32), np.full(nb, NAN, f32)
    rew[slots], val[slots] = g.standard_normal(n).astype(f32), (2 * g.standard_normal(n)).astype(f32)
    old = g.standard_normal(n).astype(f32)
    old[g.random(n) < 0.5] = NAN
    ret0[slots] = old
    stale = (g.random(nb) < 0.5).astype(np.uint8)
    steps = [[int(sel[offs[s] + i]) for s in range(int(lens[i]))] for i in range(F)]
    boot = np.zeros(nb, bool)
    for i in range(F):
        if last[i]:
            boot[steps[i][-1]] = True
    b0 = int(np.flatnonzero(boot)[0])
    stale[b0], ret0[b0] = 1, 0.25                # a bootstrap step that is stale with a finite old return still becomes NaN
    first = info["sequence_starts"]
    key = {(int(env[first[i]]), int(ep[first[i]])): i for i in range(F)}
    nxt = [key.get((int(env[first[i]]), int(ep[first[i]]) + 1)) for i in range(F)]
    return NS(F=F, nb=nb, named=named, rew=rew, val=val, ret0=ret0, stale=stale, steps=steps, last=last.astype(np.uint8), boot=boot,
              nxt=nxt, packed=np.concatenate([sel, offs, lens]).astype(np.int32), nsel=len(sel), noffs=len(offs))


def ver_ref(d, gamma=GAMMA, tau=TAU, *, overwrite_stale=False, across_ends=False):
    """The numpy float64 loop of the reference storage, rounded to float32 on assignment."""
    ret = d.ret0.copy()
    for i, st in enumerate(d.steps):
        gae = 0.0
        lastv = f64(d.val[d.steps[d.nxt[i]][0]]) if across_ends and d.nxt[i] is not None else 0.0
        for s in reversed(range(len(st))):
            b = st[s]
            v = f64(d.val[b])
            gae = (f64(d.rew[b]) + gamma * lastv - v) + tau * gamma * gae
            bt = bool(d.last[i]) and s == len(st) - 1
            if bt:
                gae = 0.0
            if overwrite_stale or not d.stale[b] or not np.isfinite(ret[b]):
                ret[b] = f32(gae + v)
            if bt:
                ret[b] = NAN
            lastv = v
    return ret


def within_one_ulp(got, ref):
    n = np.isnan(ref)
    if not np.array_equal(np.isnan(got), n):
        return False, 0
    diff = np.abs(got[~n].astype(f64) - ref[~n].astype(f64))
    return bool((diff <= np.spacing(np.abs(ref[~n])).astype(f64)).all()), int((diff != 0).sum())


def test_ver_reference_properties_and_wrong_variants():
    for name in VER_NAMES:
        d = ver_data(name)
        ref = ver_ref(d)
        keep = d.named & (d.stale != 0) & np.isfinite(d.ret0) & ~d.boot
        assert np.array_equal(ref[keep].view(np.int32), d.ret0[keep].view(np.int32))
        assert np.isnan(ref[d.boot]).all() and np.isnan(ref[~d.named]).all()
        assert not np.isnan(ref[d.named & ~d.boot]).any()
        if name in ("F63", "F64", "F65", "F130"):
            assert keep.sum() > 3 and (d.named & (d.stale != 0) & np.isnan(d.ret0) & ~d.boot).sum() > 3
            assert not within_one_ulp(ver_ref(d, overwrite_stale=True), ref)[0], "a recursion that overwrites stale steps"
            assert not within_one_ulp(ver_ref(d, across_ends=True), ref)[0], "a recursion that bootstraps across a sequence end"


def test_ver_reference_equals_gae_reference_on_one_full_sequence():
    """One environment, one fresh sequence of T + 1 steps: its last step is the bootstrap, the others are GAE with all masks 1 and
    next_value = the last step's value."""
    Tn = 40
    g = rng(7)
    rew, val = g.standard_normal(Tn + 1).astype(f32), g.standard_normal(Tn + 1).astype(f32)
    d = NS(steps=[list(range(Tn + 1))], last=np.ones(1, np.uint8), nxt=[None], rew=rew, val=val, ret0=np.full(Tn + 1, NAN, f32),
           stale=np.zeros(Tn + 1, np.uint8))
    ver = ver_ref(d)
    gd = NS(r=rew.reshape(-1, 1).copy(), v=val.reshape(-1, 1).copy(), m=np.ones((Tn + 1, 1), np.uint8), nv=val[Tn:].copy())
    gae, _ = gae_ref(gd, Tn, 1, 1, round_hp=False)
    assert np.isnan(ver[Tn])
    assert np.array_equal(ver[:Tn], gae.v[:Tn, 0].astype(f32))


@gpu
@pytest.mark.parametrize("name", VER_NAMES)
def test_ver_compute_returns(L, name):
    d = ver_data(name)
    ref = ver_ref(d)
    r0 = guard(d.ret0)

    def run():
        rew, val, st, ret, pk, lm = dev(d.rew), dev(d.val), dev(d.stale), r0.cuda(), dev(d.packed), dev(d.last)
        base = pk.data_ptr()
        P(pk)
        rc = L.hab_ver_compute_returns(P(rew), P(val), P(st), PB(ret), C.c_void_p(base), C.c_void_p(base + 4 * d.nsel),
                                       C.c_void_p(base + 4 * (d.nsel + d.noffs)), P(lm), d.F, GAMMA, TAU, S())
        torch.cuda.synchronize()
        assert rc == 0
        return dict(ret=ret.cpu())
    o = twice(run)
    written = d.named & ((d.stale == 0) | ~np.isfinite(d.ret0) | d.boot)
    assert untouched(r0, o["ret"], written), "a kept return, a slot no sequence names or a guard changed"
    ok, ndiff = within_one_ulp(body(o["ret"]).numpy(), ref)
    print(f"hab_ver_compute_returns {name}: {ndiff} of {int(d.named.sum())} elements differ from the rounded float64 loop")
    k = "hab_ver_compute_returns (share of elements not bit-equal)"
    WORST[k] = max(WORST.get(k, 0.0), ndiff / int(d.named.sum()))
    assert ok, "NaN pattern differs or a value is more than one float32 ulp off"


# ================================================================================================
# hab_ver_is_coeffs
# ================================================================================================
def isc_cases():
    for n in (1, 255, 256, 257, 4096):
        g = rng(8, n)
        yield n, "one_env", np.full(n, 2, np.int64), 5
        yield n, "one_each", g.permutation(n).astype(np.int64), n
        ids = g.integers(-1, 8, n).astype(np.int64)      # -1 and num_envs = 7 are out of range: coefficient 1.0, not counted
        yield n, "mixed", ids, 7


@gpu
def test_ver_is_coeffs(L):
    num_steps = 31
    for n, kind, ids, num_envs in isc_cases():
        ok = (ids >= 0) & (ids < num_envs)
        counts = np.bincount(ids[ok], minlength=num_envs).astype(np.int32)
        exp = np.ones(n, f32)
        exp[ok] = f32(num_steps + 1) / counts[ids[ok]].astype(f32)
        c0, o0 = guard(torch.full((num_envs,), 12345, dtype=torch.int32), ISENT), guard(nans(n))

        def run():
            i, c, o = dev(ids), c0.cuda(), o0.cuda()
            rc = L.hab_ver_is_coeffs(P(i), n, num_envs, num_steps, PB(c), PB(o), S())
            torch.cuda.synchronize()
            assert rc == 0
            return dict(c=c.cpu(), o=o.cpu())
        o = twice(run)
        assert untouched(c0, o["c"], np.ones(num_envs, bool)) and untouched(o0, o["o"], np.ones(n, bool)), (n, kind)
        assert torch.equal(body(o["c"]), T(counts)), (n, kind, "counts")
        assert same_bits(body(o["o"]), T(exp)), (n, kind, "coefficients are not numpy's float32 quotient")


# ================================================================================================
# hab_sample_actions
# ================================================================================================
@functools.lru_cache(maxsize=None)
def sample_data(n, A):
    g = rng(9, n, A)
    p = g.random((n, A)).astype(f32)
    p /= p.sum(1, keepdims=True)
    q = g.exponential(1.0, (n, A)).astype(f32) + f32(1e-3)
    p[g.random((n, A)) < 0.2] = 0.0                       # zero-probability classes
    if A >= 4:
        for i in range(0, n, 3):                          # exact ties of p / q that are the row's maximum: the first index wins
            j, k = sorted(g.choice(A, 2, replace=False))
            p[i, j] = p[i, k] = 0.5
            q[i, j] = q[i, k] = 2.0 ** -20
        for i in range(1, n, 3):                          # tied maxima of p itself for deterministic = 1
            j, k = sorted(g.choice(A, 2, replace=False))
            p[i, j] = p[i, k] = 2.0
    if n > 2:
        p[2] = 0.0                                        # a row of zeros: every quotient ties at 0
    return p, q


@gpu
@pytest.mark.parametrize("A", (1, 4, 18))
def test_sample_actions(L, A):
    for n in (1, 63, 64, 65):
        p, q = sample_data(n, A)
        for det in (0, 1):
            exp = np.argmax(p if det else p / q, axis=1).astype(np.int64)
            a0 = guard(torch.full((n,), ISENT, dtype=torch.int64), ISENT)

            def run():
                pp, qq, a = dev(p), dev(q), a0.cuda()
                rc = L.hab_sample_actions(P(pp), None if det else P(qq), PB(a), n, A, det, S())
                torch.cuda.synchronize()
                assert rc == 0
                return dict(a=a.cpu())
            o = twice(run)
            assert untouched(a0, o["a"], np.ones(n, bool))
            assert torch.equal(body(o["a"]), T(exp)), (n, A, det)


def test_sample_data_has_ties_and_zeros():
    p, q = sample_data(65, 18)
    s = p / q
    assert ((s == s.max(1, keepdims=True)).sum(1) >= 2).sum() >= 20 and (p == 0).any()
    assert ((p == p.max(1, keepdims=True)).sum(1) >= 2).sum() >= 20


# ================================================================================================
# Refusals decided before any launch: HAB_ERR_ARG, nothing written.  Every pointer is a real buffer of ample size.
# ================================================================================================
@gpu
def test_refusals_leave_outputs_untouched(L):
    n = 64
    f0 = nans(4 * n)
    fb = [f0.cuda() for _ in range(12)]
    i64 = torch.full((n,), ISENT, dtype=torch.int64).cuda()
    i32 = torch.full((4 * n,), ISENT, dtype=torch.int32).cuda()
    u8 = torch.ones(n, dtype=torch.uint8).cuda()
    sc = torch.full((SCRATCH,), NAN, dtype=torch.float64).cuda()
    f = [P(x) for x in fb]
    s = S()
    calls = []
    for count in (0, -1):
        calls.append(L.hab_advantages(f[0], f[1], f[2], count, 1, None, f[3], s))
    calls.append(L.hab_advantages(f[0], f[1], f[2], n, 5, f[4], f[3], s))
    calls.append(L.hab_advantages(f[0], f[1], f[2], n, 3, None, f[3], s))
    calls.append(L.hab_advantages(f[0], f[1], f[2], n, 4, None, f[3], s))
    calls.append(L.hab_advantages(f[0], f[1], f[2], n, 2, None, None, s))
    calls.append(L.hab_advantages(f[0], f[1], f[2], n, 4, f[4], None, s))
    for B in (0, -3):
        calls.append(L.hab_ppo_loss(*f[0:7], None, B, 0.2, 0.5, 0.01, 1, f[7], f[8], f[9], f[10], s))
        calls.append(L.hab_ppo_loss_ver(*f[0:7], None, B, 0.2, 0.5, 0.01, 1, None, None, None, 0, None, 0.0, f[7], f[8], f[9], f[10], s))
    for step in (0, -1):
        calls.append(L.hab_clip_adam_step(f[0], f[1], f[2], f[3], n, P(sc), 1024, 1.0, 0.5, LR, B1, B2, EPS, step, f[4], s))
        calls.append(L.hab_lagrange_adam_step(f[0], f[1], f[2], f[3], 1.0, LR, B1, B2, EPS, step, -1.0, 0.0, f[4], s))
    calls.append(L.hab_clip_adam_step(f[0], f[1], f[2], f[3], 0, P(sc), 1024, 1.0, 0.5, LR, B1, B2, EPS, 1, f[4], s))
    calls.append(L.hab_clip_adam_step(f[0], f[1], f[2], f[3], n, P(sc), 0, 1.0, 0.5, LR, B1, B2, EPS, 1, f[4], s))
    calls.append(L.hab_clip_adam_step(PB(fb[0], 1), f[1], f[2], f[3], n, P(sc), 1024, 1.0, 0.5, LR, B1, B2, EPS, 1, f[4], s))
    for F in (0, -1):
        calls.append(L.hab_ver_compute_returns(f[0], f[1], P(u8), f[2], P(i32), P(i32), P(i32), P(u8), F, GAMMA, TAU, s))
    for m in (0, -1):
        calls.append(L.hab_ver_is_coeffs(P(i64), m, 4, 31, P(i32), f[5], s))
        calls.append(L.hab_sample_actions(f[0], f[1], P(i64), m, 4, 0, s))
    calls.append(L.hab_compute_returns(f[0], f[1], P(u8), f[2], f[3], 3, 0, GAMMA, TAU, 1, 0, s))
    calls.append(L.hab_compute_returns(f[0], f[1], P(u8), f[2], f[3], -1, 4, GAMMA, TAU, 1, 1, s))
    torch.cuda.synchronize()
    assert calls == [HAB_ERR_ARG] * len(calls), calls
    for x in fb:
        assert same_bits(x.cpu(), f0)
    assert bool((i64 == ISENT).all()) and bool((i32 == ISENT).all()) and bool(torch.isnan(sc).all())
