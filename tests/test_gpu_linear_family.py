"""hab_linear_fwd / _dgrad / _wgrad, hab_colsum, hab_transpose2d and hab_repack_flatten_weight against float64 on the CPU, at the operand
layouts, options and dispatch edges the engine uses: every epilogue option (bias, ReLU, accumulate, ReLU mask with its own row stride,
the NHWC-flatten -> NCHW-flatten column permutation), leading dimensions and reduction lengths that are no multiple of 4, the tiny tiles
against the width classes (M = 64 / 65), the 96-row weight-gradient tiles, every split-K form (none, narrow reduce, wide reduce, limited
by the workspace) and the dense kernel, each under matrix path 0 (fp32 MFMA tiles), 2047 (default) and 4095 (MP_DENSE_ALL).

Every GPU case: operand padding is NaN (it must never contribute), the output is pre-filled with NaN (or `old` and 7.0 in the padding
when it accumulates) and its padding must come back bit for bit, the workspace is longer than the ws_floats passed and its tail must
stay untouched, its head is re-randomised before each call, and every call is made twice and must reproduce its bits.

Error bars (the project's, tests/test_gpu_bf3.py): max-norm relative error against float64 below 3e-6 for reductions of at most 1200,
which is also the per-element bar |got - ref| <= 3e-6 max|ref|; modes 2047 and 4095 additionally e <= 2 e(mode 0) + 2e-7.  Reductions
longer than 1200: per element |got - ref| <= (K + 8) 2^-24 sum_k |a_k b_k| (Higham's bound for any summation order; + 8 for bias,
accumulate and the split's dropped terms), computed in float64 from the operands.  The CPU self-checks at the end hold a float32
evaluation of every case to half of these allowances."""
import ctypes as C
import functools
import os
import subprocess
from types import SimpleNamespace as NS

import pytest
import torch

from habitat_amd import _lib


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


_KEEP = []


def P(t):
    """Device pointer of a tensor for a ctypes call (kept alive for the next few dozen calls, see tests/test_gpu_bf3.py)."""
    if t is None:
        return None
    _KEEP.append(t)
    if len(_KEEP) > 96:
        del _KEEP[:48]
    return C.c_void_p(t.data_ptr())
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _with_path(L, mode, fn):
    prev = L.hab_set_matrix_path(-1)
    try:
        L.hab_set_matrix_path(mode)
        return fn()
    finally:
        L.hab_set_matrix_path(prev)


def err_vs(ref64, y):
    ref = ref64.double()
    return ((y.double().cpu() - ref).abs().max() / ref.abs().max()).item()


MODES = (0, 2047, 4095)
NAN = float("nan")
AMPLE = 1 << 22        # ws_floats of an "ample" workspace
WS_TAIL = 1 << 22      # floats behind ws_floats that must stay untouched (more than any case's unlimited split plan needs)
TAILV = -3.0
HAB_ERR_ARG = -1
U = 2.0 ** -24
WORST = {}             # (section, mode) -> worst max-norm relative error seen in this run


@pytest.fixture(scope="module")
def WS():
    buf = torch.full((AMPLE + WS_TAIL,), TAILV, device="cuda")
    yield buf
    for k in sorted(WORST):
        print("worst error %-8s mode %-5s %.3g" % (k[0], k[1], WORST[k]))


def ws_call(WS, ws, launch):
    """launch(ws pointer, ws_floats) with the head of the workspace re-randomised and the tail checked afterwards; ws None: no workspace."""
    if ws is None:
        return launch(None, 0)
    assert 0 <= ws <= AMPLE
    WS[:ws].normal_()
    rc = launch(P(WS), ws)
    assert bool((WS[ws:] == TAILV).all()), "the launch wrote behind ws_floats"
    WS[:ws] = TAILV
    return rc


# ------------------------------------------------------------------------------------------------
# The dispatcher in Python (csrc/gemm_ops.hip run_igemm / by_width, csrc/igemm.h igemm_plan, csrc/dense_bf3.h dense_bf3_ok /
# dense_bf3_splits): the case tables state tile and split count, test_case_tables_match_the_dispatch_rules holds them to these rules.
# ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def rows_fit(M, rows, other):
    return M % rows == 0 or cdiv(M, rows) * rows < cdiv(M, other) * other


def igemm_tile(M, N, wg):
    """(BM, BN).  M <= 64: igemm_launch<1,1,2,1> / <1,1,2,2> / <1,2,2,2> in EVERY mode (the split-bf16 tiles need p.M > 64); else
    by_width<WG>: Tile<2,1,4,1> / <1,2,4,1> / 128 x 128, and for weight gradients the 96-row Tile<1,1,3,1> / <1,2,3,1> where rows_fit."""
    if M <= 64:
        return (64, 32) if N <= 32 else (64, 64) if N <= 64 else (64, 128)
    if N <= 32:
        return (96, 32) if wg and rows_fit(M, 96, 256) else (256, 32)
    if N <= 64:
        return (96, 64) if wg and rows_fit(M, 96, 128) else (128, 64)
    return (128, 128)


def igemm_splits(tile, M, N, K, target, ws):
    """igemm_plan: enough splits for `target` workgroups (256 forward and data gradient, 1024 weight gradient), at most one per
    32-deep k-tile, at most what fits ws_floats at (M + 1) * N floats per slab; then equal runs of k-tiles."""
    tiles = cdiv(M, tile[0]) * cdiv(N, tile[1])
    s = cdiv(target, tiles) if tiles < target else 1
    kt = cdiv(K, 32)
    s = min(s, kt, 4096)
    while s > 1 and s * (M + 1) * N > (ws or 0):
        s -= 1
    return cdiv(K, cdiv(kt, s) * 32)


def dense_ok(M, N, K, lda, ldb, aligned, a_ic, b_ic):
    return (M >= 256 and N >= 128 and K >= 256 and K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0 and aligned
            and not (a_ic and M % 4) and not (b_ic and N % 4))


def dense_splits(M, N, K, ws):
    nt = cdiv(M, 256) * cdiv(N, 128)
    if nt >= 128 or ws is None:
        return 1
    s = min(256 // nt, K // 32 // 4)
    while s > 1 and s * M * N > ws:
        s -= 1
    return max(s, 1)


# ------------------------------------------------------------------------------------------------
# Case data: float32 operands in their padded storage, float64 reference, built once per case and shared by the GPU test and the CPU
# self-check.  Fields: ops {name: (flat storage, offset of the first element)}, out0 (flat output storage before the call), rows /
# width / ld of the output, ref [rows][width] float64, K (reduction length), S (sum_k |a_k b_k|), zero (elements that must be +0.0).
# ------------------------------------------------------------------------------------------------
def heavy(g, *shape):
    return torch.randn(*shape, generator=g) * torch.rand(*shape, generator=g).pow(3) * 10


def store(t, ld, off=0):
    """[rows][cols] tensor in a NaN-filled flat storage with row stride ld, first element at `off`."""
    rows, cols = t.shape
    assert ld >= cols
    flat = torch.full((off + rows * ld,), NAN)
    flat[off:].view(rows, ld)[:, :cols] = t
    return flat, off


def out_storage(rows, width, ld, old):
    """NaN everywhere when nothing is accumulated; else `old` with 7.0 in the padding columns."""
    assert ld >= width
    flat = torch.full((rows * ld,), NAN if old is None else 7.0)
    if old is not None:
        flat.view(rows, ld)[:, :width] = old
    return flat


def relu_mask(g, rows, ld):
    """~40 % non-positive entries, exact +0.0 and -0.0 among them; the padding columns are random too (a wrong row stride reads them)."""
    m = torch.randn(rows, ld, generator=g).abs() + 0.01
    r = torch.rand(rows, ld, generator=g)
    m[r < 0.4] *= -1
    m[r < 0.2] = -0.0
    m[r < 0.1] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def fwd_data(M, N, K, ldx, ldw, xoff, bias, relu, acc, ldy, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    x, w = heavy(g, M, K), torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    old = torch.randn(M, N, generator=g) if acc else None
    ref = x.double() @ w.double().t()
    if bias:
        ref = ref + b.double()
    if acc:
        ref = ref + old.double()
    if relu:
        ref = ref.relu()
    d = NS(ops={"x": store(x, ldx, xoff), "w": store(w, ldw)}, out0=out_storage(M, N, ldy, old), rows=M, width=N, ld=ldy, ref=ref, K=K,
           zero=None, S=x.double().abs() @ w.double().abs().t())
    if bias:
        d.ops["b"] = (b, 0)
    return d


@functools.lru_cache(maxsize=None)
def dgrad_data(M, n_in, n_out, lddy, ldw, ldmask, acc, lddx, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    dy, w = heavy(g, M, n_out), torch.randn(n_out, n_in, generator=g) / n_out ** 0.5
    old = torch.randn(M, n_in, generator=g) if acc else None
    ref = dy.double() @ w.double()
    if acc:
        ref = ref + old.double()
    d = NS(ops={"dy": store(dy, lddy), "w": store(w, ldw)}, out0=out_storage(M, n_in, lddx, old), rows=M, width=n_in, ld=lddx, K=n_out,
           zero=None, S=dy.double().abs() @ w.double().abs())
    if ldmask:
        m = relu_mask(g, M, ldmask)
        d.ops["mask"] = (m.flatten(), 0)
        d.zero = ~(m[:, :n_in] > 0)
        ref = ref * (m[:, :n_in] > 0)
    d.ref = ref
    return d


@functools.lru_cache(maxsize=None)
def wgrad_data(rows, n_out, n_in, lddy, ldx, lddw, perm_c, perm_hw, acc, seed):
    g = torch.Generator().manual_seed(3000 + seed)
    dy = torch.randn(rows, n_out, generator=g) * torch.rand(rows, n_out, generator=g).pow(3)
    x = heavy(g, rows, n_in)
    old = torch.randn(n_out, n_in, generator=g) if acc else None
    ref, sab = dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs()
    if perm_c:  # column hw * C + c of x is column c * HW + hw of the reference weight
        assert n_in == perm_c * perm_hw
        ref, sab = (t.view(n_out, perm_hw, perm_c).transpose(1, 2).reshape(n_out, n_in) for t in (ref, sab))
    if acc:
        ref = ref + old.double()
    return NS(ops={"dy": store(dy, lddy), "x": store(x, ldx)}, out0=out_storage(n_out, n_in, lddw, old), rows=n_out, width=n_in, ld=lddw,
              ref=ref, K=rows, zero=None, S=sab)


@functools.lru_cache(maxsize=None)
def colsum_data(M, N, lda, aoff, acc):
    g = torch.Generator().manual_seed(4000 + 7 * M + N)
    a = heavy(g, M, N)
    old = torch.randn(1, N, generator=g) if acc else None
    ref = a.double().sum(0, keepdim=True)
    if acc:
        ref = ref + old.double()
    return NS(ops={"a": store(a, lda, aoff)}, out0=out_storage(1, N, N, old), rows=1, width=N, ld=N, ref=ref, K=M, zero=None,
              S=a.double().abs().sum(0, keepdim=True))


def view_of(d, name, rows, cols, ld):
    flat, off = d.ops[name]
    return flat[off:off + rows * ld].view(rows, ld)[:, :cols]


def check_out(d, flat, scale=1.0):
    """Padding bit for bit, masked elements +0.0, error bar (times `scale`, 0.5 for the CPU self-check); returns the max-norm error."""
    out, out0 = flat.view(d.rows, d.ld), d.out0.view(d.rows, d.ld)
    assert torch.equal(out[:, d.width:].contiguous().view(torch.int32), out0[:, d.width:].contiguous().view(torch.int32)), "padding columns written"
    got = out[:, :d.width]
    if d.zero is not None:
        assert bool((got[d.zero].contiguous().view(torch.int32) == 0).all()), "a masked element is not +0.0"
    diff = (got.double() - d.ref).abs()
    assert not torch.isnan(diff).any(), "an output element was not written (or an operand's padding was read)"
    e = err_vs(d.ref, got)
    if d.K <= 1200:
        assert e < 3e-6 * scale, e
        assert float(diff.max()) <= 3e-6 * scale * float(d.ref.abs().max())
    else:
        bound = scale * (d.K + 8) * U * d.S
        assert bool((diff <= bound).all()), float((diff / bound.clamp_min(1e-300)).max())
    return e


def dev_ops(d):
    """Operands on the device: name -> view that starts at the operand's first element (the storage stays alive through the view)."""
    return {k: flat.cuda()[off:] for k, (flat, off) in d.ops.items()}


def run_modes(L, WS, section, d, launch, ws, modes=MODES, note=True):
    """launch(dev, out, ws pointer, ws_floats) -> rc under each mode, twice: checks every result, reproducibility and the path-versus-
    path criterion; returns {mode: flat CPU output}."""
    dev = dev_ops(d)
    outs, errs = {}, {}

    def once():
        out = d.out0.cuda()
        _lib.check(ws_call(WS, ws, lambda wp, wn: launch(dev, out, wp, wn)))
        return out.cpu()

    for mode in modes:
        a = _with_path(L, mode, once)
        b = _with_path(L, mode, once)
        assert same(a, b), ("not reproducible", mode)
        outs[mode], errs[mode] = a, check_out(d, a)
        if note:
            WORST[(section, mode)] = max(WORST.get((section, mode), 0.0), errs[mode])
    if 0 in errs:
        for mode in modes:
            assert errs[mode] <= 2 * errs[0] + 2e-7, (mode, errs)
    return outs


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# 1. hab_linear_fwd
# ------------------------------------------------------------------------------------------------
def FW(M, N, K, ldx=0, ldw=0, xoff=0, bias=0, relu=0, acc=0, ldy=0, ws=AMPLE, seed=0, tile=None, sp=None, dense=0):
    return NS(M=M, N=N, K=K, ldx=ldx or K, ldw=ldw or K, xoff=xoff, bias=bias, relu=relu, acc=acc, ldy=ldy or N, ws=ws, seed=seed,
              tile=tile, sp=sp, dense=dense)


# LinearFwdProb is r-contiguous in both operands (RC): target 256 workgroups; under MP_RC and M > 64 the split-bf16 tiles of by_width,
# else the fp32 tiles -- the tiny ones for M <= 64.  tile = (BM, BN); sp = the split count igemm_plan reaches: min(ceil(256 / tiles),
# ceil(K / 32), what ws_floats holds at (M + 1) N floats per slab), then ceil(K / k_per_split).  sp >= 16 takes the WIDE reduction
# pass, 2..15 the narrow one.  vec = 0 (scalar gathers) where K, ldx or ldw is no multiple of 4 or x is not 16-byte aligned.
# dense: dense_bf3_ok holds (M >= 256, N >= 128, K >= 256, K % 32 == 0, aligned operands), so mode 4095 runs dense_bf3_kernel, with
# dense_bf3_splits = min(256 / tiles(256 x 128), K / 32 / 4) = min(256 / 4, 9) = 9 slabs when it has a workspace.
_SPLIT = dict(M=96, N=48, K=1024, bias=1, relu=1, seed=12, tile=(128, 64))  # one 128 x 64 tile, 32 k-tiles: the plan wants 32 splits
FWD = {
    # M <= 64: tiny tiles in every mode
    # N = 1, 16 k-tiles -> 16 slabs, WIDE.  One output element: the max-norm bar is that element's own relative error, so the seed is one
    # at which the dot product does not cancel (test_cases_are_well_conditioned)
    "critic_rollout": FW(1, 1, 512, bias=1, seed=4, tile=(64, 32), sp=16),
    "below_one_ktile": FW(5, 20, 7, relu=1, tile=(64, 32), sp=1),                          # K = 7: one ragged k-tile, scalar gathers
    "tiny_n33": FW(64, 33, 200, bias=1, relu=1, acc=1, ldy=36, tile=(64, 64), sp=7),       # 7 k-tiles -> 7 slabs, narrow
    "m64_n100": FW(64, 100, 96, bias=1, seed=4, tile=(64, 128), sp=3),
    # M > 64: width classes
    "m65_n100": FW(65, 100, 96, bias=1, seed=4, tile=(128, 128), sp=3),
    "n30_ktail": FW(300, 30, 1000, relu=1, ldy=32, tile=(256, 32), sp=32),                 # K % 32 = 8: vector fetch with a tail; 2 tiles -> 32 slabs
    "n64_ktail": FW(129, 64, 612, bias=1, acc=1, tile=(128, 64), sp=20),                   # K % 32 = 4; 2 tiles, 20 k-tiles
    "n70_kscalar": FW(131, 70, 301, bias=1, relu=1, tile=(128, 128), sp=10),               # K % 4 = 1: scalar fetch; 2 tiles, 10 k-tiles
    "ldx_odd": FW(100, 40, 128, ldx=129, acc=1, tile=(128, 64), sp=4),
    "ldw_odd": FW(100, 40, 128, ldw=130, bias=1, ldy=41, tile=(128, 64), sp=4),
    "x_off_by_one_float": FW(100, 40, 128, ldx=132, xoff=1, relu=1, tile=(128, 64), sp=4),
    # split-K of one tile
    "split_none": FW(ws=None, sp=1, **_SPLIT),
    "split_ws_below_two_slabs": FW(ws=2 * 97 * 48 - 1, sp=1, **_SPLIT),
    "split_ws_5": FW(ws=5 * 97 * 48, sp=5, **_SPLIT),                                      # 5 slabs fit: runs of 7 k-tiles -> 5, narrow
    "split_ws_20": FW(ws=20 * 97 * 48, sp=16, **_SPLIT),                                   # 20 slabs fit: runs of 2 k-tiles -> 16, WIDE
    "split_ample": FW(sp=32, **_SPLIT),
    # K >= 2048 and the 128 x 128 tile: MP_WS selects the producer / consumer kernel; 2 tiles, 65 k-tiles -> 65 slabs
    "long_k_ragged": FW(130, 70, 2052, bias=1, tile=(128, 128), sp=65),
    # accepted by dense_bf3_ok: 6 igemm tiles -> min(43, 36 k-tiles) = 36 slabs under 0 and 2047; dense_bf3_kernel under 4095
    "dense_split": FW(300, 132, 1152, bias=1, relu=1, acc=1, ldy=136, seed=18, tile=(128, 128), sp=36, dense=1),
    "dense_no_split": FW(300, 132, 1152, bias=1, relu=1, acc=1, ldy=136, ws=None, seed=18, tile=(128, 128), sp=1, dense=1),
}


def fwd_build(c):
    return fwd_data(c.M, c.N, c.K, c.ldx, c.ldw, c.xoff, c.bias, c.relu, c.acc, c.ldy, c.seed)


def fwd_launch(L, c):
    return lambda dev, out, wp, wn: L.hab_linear_fwd(P(dev["x"]), c.ldx, P(dev["w"]), c.ldw, P(dev.get("b")), P(out), c.ldy, c.M, c.N, c.K,
                                                     c.relu, c.acc, wp, wn, S())


def fwd_cpu32(c, d):
    y = view_of(d, "x", c.M, c.K, c.ldx) @ view_of(d, "w", c.N, c.K, c.ldw).t()
    if c.bias:
        y = y + d.ops["b"][0]
    return y


def check_dispatch(c, outs, dense, what):
    """Which kernel ran, by its bits: M <= 64 -> the same tiny fp32 tile in every mode; M > 64 -> mode 2047 is not mode 0's kernel;
    mode 4095 differs from 2047 exactly where the dense kernel takes the shape."""
    if c.M <= 64:
        assert same(outs[0], outs[2047]) and same(outs[0], outs[4095]), what + ": M <= 64 must run the tiny fp32 tile in every mode"
        return
    assert not same(outs[0], outs[2047]), what + ": mode 2047 ran mode 0's kernel"
    if dense:
        assert not same(outs[2047], outs[4095]), what + ": mode 4095 did not select the dense kernel"
    else:
        assert same(outs[2047], outs[4095]), what + ": mode 4095 must run mode 2047's kernel where the dense kernel does not apply"


_FWD_OUTS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_linear_fwd(L, WS, name):
    c = FWD[name]
    outs = run_modes(L, WS, "fwd", fwd_build(c), fwd_launch(L, c), c.ws)
    check_dispatch(c, outs, c.dense, name)
    _FWD_OUTS[name] = outs


@pytest.mark.gpu
def test_linear_fwd_split_forms(L, WS):
    """Across cases: a workspace too small for two slabs gives the unsplit launch's bits, every real split gives other bits (its own
    summation order), and the same holds for the dense kernel under 4095.  (M = 64 against M = 65 is pinned per case by check_dispatch.)"""
    for name in ("split_none", "split_ws_below_two_slabs", "split_ws_5", "split_ws_20", "split_ample", "dense_no_split", "dense_split"):
        if name not in _FWD_OUTS:
            c = FWD[name]
            _FWD_OUTS[name] = run_modes(L, WS, "fwd", fwd_build(c), fwd_launch(L, c), c.ws)
    o = _FWD_OUTS
    for mode in MODES:
        assert same(o["split_none"][mode], o["split_ws_below_two_slabs"][mode]), mode
        for a, b in (("split_none", "split_ws_5"), ("split_ws_5", "split_ws_20"), ("split_ws_20", "split_ample")):
            assert not same(o[a][mode], o[b][mode]), (a, b, mode)
        assert not same(o["dense_no_split"][mode], o["dense_split"][mode]), mode  # 4095: dense_bf3_kernel alone against its 9 slabs


@pytest.mark.gpu
def test_linear_fwd_producer_consumer_kernel_is_bit_identical_at_a_ragged_shape(L, WS):
    c = FWD["long_k_ragged"]
    outs = run_modes(L, WS, "fwd", fwd_build(c), fwd_launch(L, c), c.ws, modes=(2047 & ~32, 2047), note=False)
    assert same(outs[2047 & ~32], outs[2047])


# ------------------------------------------------------------------------------------------------
# 2. hab_linear_dgrad
# ------------------------------------------------------------------------------------------------
def DG(M, n_in, n_out, lddy=0, ldw=0, ldmask=0, acc=0, lddx=0, ws=AMPLE, seed=0, tile=None, sp=None, dense=0):
    return NS(M=M, n_in=n_in, n_out=n_out, lddy=lddy or n_out, ldw=ldw or n_in, ldmask=ldmask, acc=acc, lddx=lddx or n_in, ws=ws, seed=seed,
              tile=tile, sp=sp, dense=dense)


# LinearDgradProb: M rows, N = n_in, reduction K = n_out; dY is r-contiguous (vec_a = 0, scalar gathers, where lddy or n_out is no
# multiple of 4), W is the k-strided operand read through col_fetch4(w, ldw, k, j, n_in): 16-byte loads where ldw % 4 == 0 and the quad
# lies inside n_in, scalar loads for the mixed last quad (n_in % 4 != 0) and for every quad where ldw % 4 != 0.  MP_IJ and M > 64 select
# the split-bf16 tiles, target 256.  A mask keeps the dense kernel out (linear_dgrad asks it only without one): 4095 must equal 2047.
# Without a mask dense_bf3_ok wants M >= 256, n_in >= 128 and % 4 == 0, n_out >= 256 and % 32 == 0.
DGRAD = {
    "m1_nout1": DG(1, 64, 1, tile=(64, 64), sp=1),                                          # critic: lddy = 1
    "m64_mixed_quad": DG(64, 30, 33, ldw=32, ldmask=35, seed=2, tile=(64, 32), sp=2),       # n_in % 4 = 2, ldw % 4 = 0; 2 k-tiles
    "m65_mixed_quad": DG(65, 30, 33, ldw=32, ldmask=35, seed=2, tile=(256, 32), sp=2),
    "m300_scalar_w": DG(300, 30, 33, ldmask=35, acc=1, lddx=33, tile=(256, 32), sp=2),      # ldw = 30: scalar branch
    "m300_nout6": DG(300, 72, 6, ldw=72, acc=1, lddx=76, tile=(128, 128), sp=1),            # n_out % 4 != 0: vec_a = 0; one k-tile
    "m300_actor": DG(300, 64, 4, lddy=8, ldmask=64, tile=(128, 64), sp=1),                  # lddy = 8 > n_out (actor head)
    "m64_n100": DG(64, 100, 40, ldmask=104, acc=1, seed=7, tile=(64, 128), sp=2),
    "m65_n100": DG(65, 100, 40, ldmask=104, acc=1, seed=7, tile=(128, 128), sp=2),
    "mask_dense_shape": DG(300, 128, 512, ldmask=132, seed=9, tile=(128, 128), sp=16),      # 3 tiles -> min(86, 16 k-tiles) = 16, WIDE
    "mask_dense_shape_acc": DG(300, 128, 512, ldmask=132, acc=1, lddx=132, seed=9, tile=(128, 128), sp=16),
    "dense_shape": DG(300, 128, 512, seed=9, tile=(128, 128), sp=16, dense=1),              # no mask: dense_bf3_kernel under 4095
    "mask_no_ws": DG(300, 30, 33, ldw=32, ldmask=35, ws=None, tile=(256, 32), sp=1),
}


def dgrad_build(c):
    return dgrad_data(c.M, c.n_in, c.n_out, c.lddy, c.ldw, c.ldmask, c.acc, c.lddx, c.seed)


def dgrad_launch(L, c):
    return lambda dev, out, wp, wn: L.hab_linear_dgrad(P(dev["dy"]), c.lddy, P(dev["w"]), c.ldw, P(dev.get("mask")), c.ldmask, P(out), c.lddx,
                                                       c.M, c.n_in, c.n_out, c.acc, wp, wn, S())


def dgrad_cpu32(c, d):
    return view_of(d, "dy", c.M, c.n_out, c.lddy) @ view_of(d, "w", c.n_out, c.n_in, c.ldw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DGRAD))
def test_linear_dgrad(L, WS, name):
    """dX = (old + dY W) * (mask > 0): LinearDgradProb::epi_store adds the old value first and then zeroes where the mask is not
    positive, so a masked element is +0.0 whatever it held; the mask is read with its own row stride ldmask."""
    c = DGRAD[name]
    outs = run_modes(L, WS, "dgrad", dgrad_build(c), dgrad_launch(L, c), c.ws)
    check_dispatch(c, outs, c.dense, name)


# ------------------------------------------------------------------------------------------------
# 3. hab_linear_wgrad
# ------------------------------------------------------------------------------------------------
def WG(rows, n_out, n_in, lddy=0, ldx=0, lddw=0, perm=(0, 0), acc=0, ws=AMPLE, seed=0, tile=None, sp=None):
    return NS(rows=rows, n_out=n_out, n_in=n_in, lddy=lddy or n_out, ldx=ldx or n_in, lddw=lddw or n_in, perm=perm, acc=acc, ws=ws, seed=seed,
              tile=tile, sp=sp)


# LinearWgradProb: M = n_out, N = n_in, reduction K = rows; both operands k-strided through col_fetch4 (dY with ld = lddy, n = n_out:
# lddy = 1 and lddy = 6 take the scalar branch, lddy = 8 with n_out < 8 the mixed quad).  Weight-gradient form: target 1024 workgroups,
# by_width<true> adds the 96-row tiles where rows_fit: 96 % 96 = 0, 288 % 96 = 0, 192 % 96 = 0, 100 -> 2 * 96 = 192 < 256; 250 -> 288 >=
# 256 keeps the 256-row tile.  n_out <= 64 runs the tiny fp32 tiles in every mode.  No case here is accepted by dense_bf3_ok (n_out <
# 256 or n_in < 128 or rows < 256), so 4095 = 2047; with perm_c > 0 the permutation is applied by LinearWgradProb::epi_col -- in the
# tile's epilogue without a split, in the reduction pass (store) with one.
WGRAD = {
    "critic": WG(600, 1, 64, lddy=1, tile=(64, 64), sp=19),                                       # 19 k-tiles -> 19 slabs, WIDE
    "actor_a1": WG(33, 1, 64, lddy=8, acc=1, tile=(64, 64), sp=2),
    "actor_a3": WG(600, 3, 64, lddy=8, lddw=68, tile=(64, 64), sp=19),
    "actor_a8_one_row": WG(1, 8, 64, lddy=8, tile=(64, 64), sp=1),
    "gaussian_2a": WG(600, 6, 64, lddy=6, acc=1, tile=(64, 64), sp=19),
    "gru_gates": WG(600, 192, 64, tile=(96, 64), sp=19),
    "rows96_n32": WG(600, 96, 32, acc=1, lddw=36, tile=(96, 32), sp=19),
    "rows96_288x64": WG(33, 288, 64, tile=(96, 64), sp=2),
    "rows96_100x20": WG(600, 100, 20, tile=(96, 32), sp=19),
    "rows256_250x20": WG(600, 250, 20, acc=1, tile=(256, 32), sp=19),
    "perm32x9": WG(600, 70, 288, perm=(32, 9), seed=5, tile=(128, 128), sp=19),
    "perm32x9_acc_no_ws": WG(600, 70, 288, perm=(32, 9), acc=1, ws=None, seed=5, tile=(128, 128), sp=1),
    "perm8x5": WG(600, 50, 40, perm=(8, 5), lddw=44, seed=6, tile=(64, 64), sp=19),                # ResNet comp_c = 8: hw = 5 groups of 8 columns
    "perm8x5_acc_no_ws": WG(33, 50, 40, perm=(8, 5), acc=1, ws=None, seed=6, tile=(64, 64), sp=1),
    "perm5x8": WG(600, 70, 40, perm=(5, 8), acc=1, seed=8, tile=(96, 64), sp=19),                 # FastDiv by a non-power of two
    "deep_5000": WG(5000, 96, 32, acc=1, tile=(96, 32), sp=157),                                   # 157 k-tiles -> 157 slabs, WIDE
}


def wgrad_build(c):
    return wgrad_data(c.rows, c.n_out, c.n_in, c.lddy, c.ldx, c.lddw, c.perm[0], c.perm[1], c.acc, c.seed)


def wgrad_launch(L, c):
    return lambda dev, out, wp, wn: L.hab_linear_wgrad(P(dev["dy"]), c.lddy, P(dev["x"]), c.ldx, P(out), c.lddw, c.rows, c.n_out, c.n_in,
                                                       c.perm[0], c.perm[1], c.acc, wp, wn, S())


def wgrad_cpu32(c, d):
    dw = view_of(d, "dy", c.rows, c.n_out, c.lddy).t() @ view_of(d, "x", c.rows, c.n_in, c.ldx)
    if c.perm[0]:
        dw = dw.view(c.n_out, c.perm[1], c.perm[0]).transpose(1, 2).reshape(c.n_out, c.n_in)
    return dw


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WGRAD))
def test_linear_wgrad(L, WS, name):
    c = WGRAD[name]
    outs = run_modes(L, WS, "wgrad", wgrad_build(c), wgrad_launch(L, c), c.ws)
    check_dispatch(NS(M=c.n_out), outs, 0, name)


# ------------------------------------------------------------------------------------------------
# 4. hab_colsum
# ------------------------------------------------------------------------------------------------
# colsum: column blocks of cw = min(64, N) columns (N = 65, 130: ragged last block; N = 3: 256 % cw != 0, one idle thread), row chunks =
# min(ceil(1024 / column blocks), ceil(M / 16)) -- one for M <= 16 -- halved until chunks * N floats fit ws_floats; below N floats the
# call is refused.  No matrix path is involved: the modes must agree bit for bit.
COLSUM_N = {1: (1, 0), 3: (3, 0), 8: (8, 0), "8_off3": (8, 3), 64: (64, 0), 65: (68, 0), 130: (130, 0)}  # N -> (lda, offset in floats)
COLSUM_M = (1, 15, 17, 600, 5000)


def colsum_launch(L, M, N, lda, acc):
    return lambda dev, out, wp, wn: L.hab_colsum(P(dev["a"]), lda, M, N, P(out), acc, wp, wn, S())


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(COLSUM_N), ids=str)
def test_colsum(L, WS, key):
    N = 8 if key == "8_off3" else key
    lda, aoff = COLSUM_N[key]
    for M in COLSUM_M:
        for acc in (0, 1):
            d = colsum_data(M, N, lda, aoff, acc)
            launch = colsum_launch(L, M, N, lda, acc)
            outs = run_modes(L, WS, "colsum", d, launch, AMPLE)
            assert same(outs[0], outs[2047]) and same(outs[0], outs[4095])
            one = run_modes(L, WS, "colsum1", d, launch, N, modes=(2047,))  # exactly N floats: the `chunks >>= 1` loop ends at one chunk
            if M >= 600 and N >= 64:  # (fewer sums can agree in every bit by chance)
                assert not same(one[2047], outs[2047]), "one chunk and many gave the same bits"
            # N - 1 floats: refused, nothing written
            out = d.out0.cuda()
            dev = dev_ops(d)
            assert ws_call(WS, N - 1, lambda wp, wn: launch(dev, out, wp, wn)) == HAB_ERR_ARG
            assert same(out.cpu(), d.out0)


# ------------------------------------------------------------------------------------------------
# 5. hab_transpose2d, hab_repack_flatten_weight: bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("R,Cc", [(1, 1), (33, 31), (192, 64), (64, 192), (100, 7)])
def test_transpose2d(L, R, Cc):
    w = heavy(torch.Generator().manual_seed(R), R, Cc).cuda()
    wt = torch.full((Cc, R), NAN, device="cuda")
    _lib.check(L.hab_transpose2d(P(w), P(wt), R, Cc, S()))
    assert same(wt, w.t().contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("N,Cc,HW", [(1, 1, 1), (5, 4, 1), (64, 32, 9), (3, 8, 5)])
def test_repack_flatten_weight(L, N, Cc, HW):
    w = heavy(torch.Generator().manual_seed(N), N, Cc * HW).cuda()
    wp = torch.full((N, HW * Cc), NAN, device="cuda")
    _lib.check(L.hab_repack_flatten_weight(P(w), P(wp), N, Cc, HW, S()))
    assert same(wp, w.view(N, Cc, HW).transpose(1, 2).reshape(N, HW * Cc).contiguous())


# ------------------------------------------------------------------------------------------------
# 6. CPU self-checks: the bars are reachable by a float32 evaluation of every case (half the allowance), the references build, and the
# tables' dispatch notes follow the dispatch rules
# ------------------------------------------------------------------------------------------------
def cpu32_out(d, y, relu=0):
    """float32 result in the case's output storage, with the epilogue of the operation: + old, ReLU, mask."""
    out = d.out0.clone().view(d.rows, d.ld)
    old = out[:, :d.width]
    y = y if bool(torch.isnan(old).all()) else y + old
    if relu:
        y = y.relu()
    if d.zero is not None:
        y = torch.where(d.zero, torch.zeros(()), y)
    out[:, :d.width] = y
    return out.flatten()


@pytest.mark.parametrize("name", list(FWD))
def test_cpu_float32_meets_half_the_bar_fwd(name):
    c = FWD[name]
    d = fwd_build(c)
    check_out(d, cpu32_out(d, fwd_cpu32(c, d), c.relu), 0.5)


@pytest.mark.parametrize("name", list(DGRAD))
def test_cpu_float32_meets_half_the_bar_dgrad(name):
    c = DGRAD[name]
    d = dgrad_build(c)
    check_out(d, cpu32_out(d, dgrad_cpu32(c, d)), 0.5)


@pytest.mark.parametrize("name", list(WGRAD))
def test_cpu_float32_meets_half_the_bar_wgrad(name):
    c = WGRAD[name]
    d = wgrad_build(c)
    check_out(d, cpu32_out(d, wgrad_cpu32(c, d)), 0.5)


@pytest.mark.parametrize("key", list(COLSUM_N), ids=str)
def test_cpu_float32_meets_half_the_bar_colsum(key):
    N = 8 if key == "8_off3" else key
    lda, aoff = COLSUM_N[key]
    for M in COLSUM_M:
        for acc in (0, 1):
            d = colsum_data(M, N, lda, aoff, acc)
            check_out(d, cpu32_out(d, view_of(d, "a", M, N, lda).sum(0, keepdim=True)), 0.5)


def all_case_data():
    for table, build in ((FWD, fwd_build), (DGRAD, dgrad_build), (WGRAD, wgrad_build)):
        for name, c in table.items():
            yield name, build(c)
    for key, (lda, aoff) in COLSUM_N.items():
        for M in COLSUM_M:
            for acc in (0, 1):
                yield "colsum %s %d" % (key, M), colsum_data(M, 8 if key == "8_off3" else key, lda, aoff, acc)


def test_cases_are_well_conditioned():
    """The fixed bar is relative to max |ref|.  A float32 evaluation in any order is off by a few 2^-24 sum_k |a_k b_k| per element, so
    the bar (3e-6 = 50 * 2^-24) can only be held where max sum_k |a_k b_k| <= 16 max |ref|: three roundings of the largest partial sum
    stay under it.  This is a property of the inputs alone; the reductions above 1200 use the per-element bound and need none."""
    for name, d in all_case_data():
        if d.K <= 1200:
            assert float(d.S.max()) <= 16 * float(d.ref.abs().max()), name


# The problem functors of csrc/problems.h (operand fetches, epi_row / epi_col / epi_fetch / epi_store) executed on the host by
# tests/hostcheck (the kernels' own index math in a plain triple loop, accumulated in float64): every case of sections 1 to 3 with its
# padded layouts, NaN padding and sentinels, held to the same checks.
@pytest.fixture(scope="module")
def hc():
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "libhab_hostcheck.so")
    if not os.path.exists(so):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC",
                               os.path.join(os.path.dirname(so), "hostcheck.hip"), "-o", so])
    return C.CDLL(so)


def host_run(d, call):
    ops = {k: flat[off:] for k, (flat, off) in d.ops.items()}
    out = d.out0.clone()
    assert call(ops, out) == 0
    check_out(d, out, 0.5)


@pytest.mark.parametrize("name", list(FWD))
def test_host_functors_fwd(hc, name):
    c = FWD[name]
    host_run(fwd_build(c), lambda o, out: hc.hc_linear_fwd(P(o["x"]), c.ldx, P(o["w"]), c.ldw, P(o.get("b")), P(out), c.ldy, c.M, c.N, c.K,
                                                           c.relu, c.acc))


@pytest.mark.parametrize("name", list(DGRAD))
def test_host_functors_dgrad(hc, name):
    c = DGRAD[name]
    host_run(dgrad_build(c), lambda o, out: hc.hc_linear_dgrad(P(o["dy"]), c.lddy, P(o["w"]), c.ldw, P(o.get("mask")), c.ldmask, c.n_in, P(out),
                                                               c.lddx, c.M, c.n_in, c.n_out, c.acc))


@pytest.mark.parametrize("name", list(WGRAD))
def test_host_functors_wgrad(hc, name):
    c = WGRAD[name]
    host_run(wgrad_build(c), lambda o, out: hc.hc_linear_wgrad(P(o["dy"]), c.lddy, P(o["x"]), c.ldx, P(out), c.lddw, c.rows, c.n_out, c.n_in,
                                                               c.perm[0], c.perm[1], c.acc))


def test_case_tables_match_the_dispatch_rules():
    for name, c in FWD.items():
        tile = igemm_tile(c.M, c.N, False)
        assert (tile, igemm_splits(tile, c.M, c.N, c.K, 256, c.ws)) == (c.tile, c.sp), name
        aligned = c.xoff % 4 == 0
        assert bool(c.dense) == dense_ok(c.M, c.N, c.K, c.ldx, c.ldw, aligned, 0, 0), name
        if c.dense:
            assert dense_splits(c.M, c.N, c.K, c.ws) == (9 if c.ws else 1), name
        # what the unlimited plan would write stays inside the buffer behind ws_floats (a launch that ignored ws_floats must not fault)
        assert igemm_splits(tile, c.M, c.N, c.K, 256, 1 << 40) * (c.M + 1) * c.N <= WS_TAIL, name
    for name, c in DGRAD.items():
        tile = igemm_tile(c.M, c.n_in, False)
        assert (tile, igemm_splits(tile, c.M, c.n_in, c.n_out, 256, c.ws)) == (c.tile, c.sp), name
        assert bool(c.dense) == (not c.ldmask and dense_ok(c.M, c.n_in, c.n_out, c.lddy, c.ldw, True, 0, 1)), name
        assert igemm_splits(tile, c.M, c.n_in, c.n_out, 256, 1 << 40) * (c.M + 1) * c.n_in <= WS_TAIL, name
    for name, c in WGRAD.items():
        tile = igemm_tile(c.n_out, c.n_in, True)
        assert (tile, igemm_splits(tile, c.n_out, c.n_in, c.rows, 1024, c.ws)) == (c.tile, c.sp), name
        assert not dense_ok(c.n_out, c.n_in, c.rows, c.lddy, c.ldx, True, 1, 1), name
        assert igemm_splits(tile, c.n_out, c.n_in, c.rows, 1024, 1 << 40) * (c.n_out + 1) * c.n_in <= WS_TAIL, name
    # the issue's rows_fit outcomes
    assert [igemm_tile(m, n, True) for m, n in ((96, 32), (288, 64), (100, 20), (250, 20))] == [(96, 32), (96, 64), (96, 32), (256, 32)]
