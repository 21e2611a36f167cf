"""
The forms and limits of the input-gradient path (mbnb_linear_grad_input, csrc/grad_kernels.hip), one table.  Cases in the format of
tests/kernel_cases.py (`_c`, `case_id`) plus

  op       grad      x.grad through autograd (matmul_4bit / linear_int8 / matmul_fp8_e4m3 and .backward())
           grad_abi  mbnb_linear_grad_input through ctypes: the only way to choose the workspace and to offset dY, dX and W
           grad_t    functional._dequantize_t: the transposed dequantise pass alone
  kernel   the name; "unsupported" where the transposed pass alone must answer MBNB_ERR_UNSUPPORTED
  variant  the second string of the library's record: "grad_t <format> <T> nested|plain vec|scalar" for the pass alone,
           "grad_generic <format> <T>><O> nested|plain" for k_grad_generic, the dense GEMM's own variant on the dense path
  fmt      "4bit" (qt, bs, cs as in the kernel-name table), "int8", "fp8", "dense"
  dt xdt   the weight dtype T, and the dtype O of x (and dX) where it differs
  off      {operand: bytes}: that operand starts so many bytes off its alignment -- dy, dx, w, ws (256-byte aligned otherwise) of grad_abi;
           w and out of grad_t (out is functional.py's own allocation: placed by the plan of tests/guard.py, so under guarded_alloc only)
  ws       the workspace of grad_abi: "null", "short" (256 bytes less than the transposed weight), "nosplit" (the transposed weight alone
           on a shape the plan splits); left out: what mbnb_linear_grad_input_workspace_bytes asks for
  bias xexp bad   as in tests/kernel_cases.py; the activation is dY here

Data and host arithmetic only, importable without a GPU.  model(case) restates linear_grad_input_dispatch, grad_dense_shape,
grad_t_shape and launch_dequant_t's `vec`; the split and the GEMM's variant come from tests/gemm_variant_cases.py's restated plan.
tests/test_gpu_grad_forms.py runs every case on poisoned and on guarded buffers and holds the library's record against `kernel`,
`variant` and model(case); tests/test_grad_forms_host.py closes the table over the source.
"""
from tests.gemm_variant_cases import dense_variant, gemm_dense_plan, padded
from tests.kernel_cases import BF16_RANGE, F16_RANGE, _c

_G, _D, _DS, _T, _NO = "grad_generic", "grad_t+dense", "grad_t+dense_splitk", "grad_t", "unsupported"
DTS = ("f16", "bf16", "f32")
GRAD_GM = 4                     # rows of dX per workgroup of k_grad_generic
OPERANDS = {"grad": (), "grad_abi": ("dy", "dx", "w", "ws"), "grad_t": ("w", "out")}
PLAN_OPERANDS = {"grad": ("dx", "ws"), "grad_abi": (), "grad_t": ("out",)}      # functional.py's allocations, in order


def offset(c, operand):
    return c.get("off", {}).get(operand, 0)


def needs_plan(c):
    return any(k in PLAN_OPERANDS[c["op"]] for k in c.get("off", {}))


def fmt_word(c):
    return c.get("qt", "nf4") if c["fmt"] == "4bit" else c["fmt"]


# ------------------------------------------------------------------------------------------------ the launcher, restated
def k_weight(c):
    return padded(c["K"], c.get("bs", 64)) if c["fmt"] == "4bit" else c["K"]


def w_aligned(c):
    return offset(c, "w") % {"4bit": 4, "int8": 8, "fp8": 8, "dense": 16}[c["fmt"]] == 0


def grad_t_shape(c):
    N, K = c["N"], c["K"]
    if N <= 0 or K <= 0 or (K + 255) // 256 > 65535 or (N + 63) // 64 > 0x7FFFFFFF:
        return False
    return c.get("bs", 64) >= 8 if c["fmt"] == "4bit" else K % 8 == 0


def grad_dense_shape(c):
    M, N, K = c.get("M", 0), c["N"], c["K"]
    if c["dt"] == "f32":
        return False
    if M <= 0 or N < 128 or N % 64 != 0 or 256 * N * 2 >= 1 << 31:
        return False
    return c["fmt"] == "4bit" or K % 8 == 0


def wt_bytes(c):
    return (c["K"] * c["N"] * 2 + 255) & ~255                          # gemm_dense_wd_bytes(K, N)


def ws_query(c):
    """mbnb_linear_grad_input_workspace_bytes."""
    if not grad_dense_shape(c):
        return 0
    s = gemm_dense_plan(c["M"], c["K"], c["N"])[1]
    return wt_bytes(c) + (s * c["M"] * c["K"] * 4 if s > 1 else 0)


def ws_bytes(c):
    """What the case hands the library (None: a NULL workspace)."""
    mode = c.get("ws")
    if mode == "null":
        return None
    if mode == "short":
        return wt_bytes(c) - 256
    if mode == "nosplit":
        return wt_bytes(c)
    return ws_query(c) or None


def nested(c):
    return c["fmt"] == "4bit" and bool(c.get("cs"))


def model(c):
    """(kernel, variant) by linear_grad_input_dispatch's conditions."""
    dt, word, nest = c["dt"], fmt_word(c), "nested" if nested(c) else "plain"
    if c["op"] == "grad_t":
        if dt == "f32" or not grad_t_shape(c) or not w_aligned(c):
            return _NO, ""
        vec = c["N"] % 8 == 0 and offset(c, "out") % 16 == 0
        return _T, f"grad_t {word} {dt} {nest} {'vec' if vec else 'scalar'}"
    M, N, K = c["M"], c["N"], c["K"]
    ws = ws_bytes(c)
    dense = (grad_dense_shape(c) and (c["fmt"] != "4bit" or c.get("bs", 64) >= 32) and w_aligned(c) and ws is not None and
             offset(c, "ws") % 256 == 0 and ws >= wt_bytes(c) and offset(c, "dy") % 16 == 0 and grad_t_shape(c))
    if dense:
        fm, s = gemm_dense_plan(M, K, N)                                # the GEMM's N is the gradient's K, its contraction runs over N
        if s > 1 and ws < wt_bytes(c) + s * M * K * 4:
            s = 1
        return (_DS if s > 1 else _D), dense_variant(M, K, N, fm, s)
    return _G, f"grad_generic {word} {dt}>{c.get('xdt', dt)} {nest}"


# ------------------------------------------------------------------------------------------------ k_dequant_t
# a wave covers 64 n x 64 k, a workgroup 64 n x 256 k, a lane 8 x 8
def _t(variant, **kw):
    return _c("grad_t", _T if variant else _NO, variant=variant, **kw)


_FORMS7 = [("nf4", False), ("fp4", False), ("nf4", True), ("fp4", True), ("int8", None), ("fp8", None), ("dense", None)]


def _fmt_kw(word, cs):
    return dict(fmt="4bit", qt=word, **({"cs": True} if cs else {})) if word in ("nf4", "fp4") else dict(fmt=word)


GRAD_T = []
for _dt in ("f16", "bf16"):
    for _w, _cs in _FORMS7:            # every (T, FMT, NESTED) in both store forms: 72 x 264 (a second n-block and a second workgroup
        _n = "nested" if _cs else "plain"      # along k, one live lane row each; K_weight = 320 > K) and 100 x 200 (N % 8 = 4, K_weight = 256)
        GRAD_T += [_t(f"grad_t {_w} {_dt} {_n} vec", N=72, K=264, dt=_dt, **_fmt_kw(_w, _cs)),
                   _t(f"grad_t {_w} {_dt} {_n} scalar", N=100, K=200, dt=_dt, **_fmt_kw(_w, _cs))]
GRAD_T += [
    # one lane; one past each tile edge
    _t("grad_t nf4 f16 plain vec", N=8, K=8, dt="f16", fmt="4bit", bs=8),
    _t("grad_t int8 bf16 plain vec", N=8, K=8, dt="bf16", fmt="int8"),
    _t("grad_t dense f16 plain vec", N=8, K=8, dt="f16", fmt="dense"),
    _t("grad_t fp8 f16 plain vec", N=64, K=256, dt="f16", fmt="fp8"),
    _t("grad_t fp4 bf16 plain vec", N=64, K=256, dt="bf16", fmt="4bit", qt="fp4"),
    _t("grad_t nf4 bf16 plain scalar", N=65, K=257, dt="bf16", fmt="4bit"),
    _t("grad_t int8 f16 plain scalar", N=65, K=264, dt="f16", fmt="int8"),
    _t("grad_t dense bf16 plain scalar", N=65, K=264, dt="bf16", fmt="dense"),
    # N % 8 == 0, the output 2 bytes off 16: scalar stores by the alignment alone (against 72 x 264 above)
    _t("grad_t nf4 f16 plain scalar", N=72, K=264, dt="f16", fmt="4bit", qt="nf4", off={"out": 2}),
    _t("grad_t int8 bf16 plain scalar", N=72, K=264, dt="bf16", fmt="int8", off={"out": 2}),
    # 4-bit: K_weight > K, the last k-block cut by k >= K
    _t("grad_t nf4 f16 plain scalar", N=100, K=127, dt="f16", fmt="4bit"),
    _t("grad_t fp4 bf16 nested vec", N=72, K=127, dt="bf16", fmt="4bit", qt="fp4", cs=True),
    # nested absmax: fewer than one and more than one blocksize2 group of absmax values (200 and 1600)
    _t("grad_t nf4 bf16 nested scalar", N=100, K=128, dt="bf16", fmt="4bit", cs=True),
    _t("grad_t nf4 f16 nested scalar", N=100, K=1024, dt="f16", fmt="4bit", cs=True),
    # a NaN absmax, FP8 bytes 0x7F and 0xFF, a NaN scale
    _t("grad_t fp4 bf16 plain vec", N=72, K=264, dt="bf16", fmt="4bit", qt="fp4", bad="w"),
    _t("grad_t fp8 bf16 plain vec", N=72, K=72, dt="bf16", fmt="fp8", bad="w"),
    _t("grad_t int8 f16 plain scalar", N=100, K=72, dt="f16", fmt="int8", bad="w"),
    # int8, fp8, dense at K = 8 and 72
    _t("grad_t int8 f16 plain vec", N=72, K=8, dt="f16", fmt="int8"), _t("grad_t int8 bf16 plain vec", N=72, K=72, dt="bf16", fmt="int8"),
    _t("grad_t fp8 bf16 plain vec", N=72, K=8, dt="bf16", fmt="fp8"), _t("grad_t fp8 f16 plain vec", N=72, K=72, dt="f16", fmt="fp8"),
    _t("grad_t dense f16 plain vec", N=72, K=8, dt="f16", fmt="dense"), _t("grad_t dense bf16 plain vec", N=72, K=72, dt="bf16", fmt="dense"),
    # K % 8 for the 8-bit and dense formats: refused at 76
    _t("", N=72, K=76, dt="bf16", fmt="int8"), _t("", N=72, K=76, dt="f16", fmt="fp8"), _t("", N=72, K=76, dt="bf16", fmt="dense"),
    # the packed weight 4 and 12 bytes off 16: legal; 1 and 2 bytes off: refused (against 72 x 264 nf4 f16 above)
    _t("grad_t nf4 f16 plain vec", N=72, K=264, dt="f16", fmt="4bit", qt="nf4", off={"w": 4}),
    _t("grad_t nf4 f16 plain vec", N=72, K=264, dt="f16", fmt="4bit", qt="nf4", off={"w": 12}),
    _t("", N=72, K=264, dt="f16", fmt="4bit", qt="nf4", off={"w": 1}),
    _t("", N=72, K=264, dt="f16", fmt="4bit", qt="nf4", off={"w": 2}),
    # W 4 bytes off 8 (int8, fp8) and 8 bytes off 16 (dense): refused (against 72 x 264 above)
    _t("", N=72, K=264, dt="bf16", fmt="int8", off={"w": 4}), _t("", N=72, K=264, dt="f16", fmt="fp8", off={"w": 4}),
    _t("", N=72, K=264, dt="f16", fmt="dense", off={"w": 8}),
]
# blocksize 4 | 8 for the pass, and every blocksize up to 4096 (64 above)
GRAD_T += [_t("", N=72, K=264, dt="bf16", fmt="4bit", bs=4)]
GRAD_T += [_t("grad_t nf4 bf16 plain vec", N=72, K=264, dt="bf16", fmt="4bit", bs=_bs) for _bs in (8, 16, 32, 256, 4096)]


# ------------------------------------------------------------------------------------------------ k_grad_generic
# a thread owns one k, a workgroup 256 k and 4 rows
def _g(op, word, dt, xdt, cs=False, **kw):
    if xdt != dt:
        kw["xdt"] = xdt
    return _c(op, _G, variant=f"grad_generic {word} {dt}>{xdt} {'nested' if cs else 'plain'}", dt=dt, **_fmt_kw(word, cs), **kw)


_MS, _NS = (1, 3, 4, 5), (1, 63, 127, 160)
_KS4, _KS8 = (2, 255, 256, 257), (1, 255, 256, 257)
GENERIC = []
_i = 0
for _dt in DTS:                        # every T x O pair in each of the five formats and with nested absmax: 63 instantiations, over
    for _xdt in DTS:                   # M = 1, 3, 4, 5, K = 1 | 2, 255, 256, 257 and N = 1, 63, 127, 160
        for _w, _cs in _FORMS7:
            _K = (_KS4 if _w in ("nf4", "fp4") else _KS8)[(_i // 4) % 4]
            _op = "grad" if _w != "dense" and _K >= 8 else "grad_abi"      # autograd where the forward has a kernel for the shape too
            GENERIC.append(_g(_op, _w, _dt, _xdt, bool(_cs), M=_MS[_i % 4], N=_NS[(_i // 2) % 4], K=_K))
            _i += 1
GENERIC += [
    # each operand of the kernel off its alignment: the same form (against the first case)
    _g("grad_abi", "int8", "bf16", "bf16", M=5, N=63, K=72),
    _g("grad_abi", "int8", "bf16", "bf16", M=5, N=63, K=72, off={"dy": 2}),
    _g("grad_abi", "int8", "bf16", "bf16", M=5, N=63, K=72, off={"dx": 2}),
    _g("grad_abi", "int8", "bf16", "bf16", M=5, N=63, K=72, off={"w": 1}),
    _g("grad_abi", "nf4", "f16", "f32", M=3, N=127, K=200, off={"dy": 2, "dx": 4, "w": 1}),
    # rows of dY over binades; NaN, +Inf and -Inf rows; a poisoned weight block; bias gradients
    _g("grad", "nf4", "bf16", "bf16", M=9, N=160, K=72, xexp=BF16_RANGE, bias=True),
    _g("grad", "fp8", "f16", "f16", M=9, N=127, K=72, xexp=F16_RANGE),
    _g("grad", "int8", "bf16", "f32", M=9, N=63, K=257, xexp=BF16_RANGE, bad="x", bias=True),
    _g("grad", "fp4", "f16", "f16", M=5, N=160, K=257, bad="x"),
    _g("grad", "nf4", "f32", "f32", M=5, N=63, K=72, bad="xw", bias=True),
    _g("grad", "nf4", "bf16", "f16", M=5, N=63, K=72, bad="w"),
    _g("grad", "int8", "f16", "f16", M=5, N=100, K=72, bad="w"),
    _g("grad", "fp8", "bf16", "bf16", M=5, N=100, K=72, bad="w"),
]

# ------------------------------------------------------------------------------------------------ the dense path, each condition from both sides
def _d(op, variant, split=False, **kw):
    return _c(op, _DS if split else _D, variant=variant, **kw)


_B4 = dict(fmt="4bit", qt="nf4")
DENSE = [
    # N = 64 | 128 | 192, and 160 (N % 64 != 0 above 128); M = 1, 4, 255 -- the forward never sends the dense GEMM fewer than 256 rows
    _g("grad", "nf4", "bf16", "bf16", M=4, N=64, K=72),
    _d("grad", "dense 256x128", M=4, N=128, K=72, dt="bf16", **_B4),
    _g("grad", "nf4", "bf16", "bf16", M=4, N=160, K=72),
    _d("grad", "dense 128x128", M=4, N=192, K=72, dt="bf16", **_B4),
    _d("grad", "dense 256x128", M=1, N=128, K=72, dt="f16", fmt="int8", bias=True),
    _d("grad", "dense 128x128", M=255, N=192, K=264, dt="f16", fmt="fp8", bias=True),
    # blocksize 16 | 32
    _g("grad", "fp4", "f16", "f16", M=4, N=128, K=72, bs=16),
    _d("grad", "dense 256x128", M=4, N=128, K=72, dt="f16", fmt="4bit", qt="fp4", bs=32),
    # K % 8 for int8: 72 | 76
    _d("grad", "dense 256x128", M=4, N=128, K=72, dt="bf16", fmt="int8"),
    _g("grad", "int8", "bf16", "bf16", M=4, N=128, K=76),
    # K ragged against the GEMM's column tiles: 8, 72, 520, and K % 8 != 0 for 4-bit (scalar stores of dX)
    _d("grad", "dense 256x128", M=4, N=128, K=8, dt="f16", fmt="fp8"),
    _d("grad", "dense 128x128", M=5, N=192, K=520, dt="bf16", fmt="4bit", qt="fp4", cs=True, bias=True),
    _d("grad", "dense 256x128", M=5, N=128, K=75, dt="f16", **_B4),
    _d("grad", "dense 128x128", M=4, N=256, K=127, dt="bf16", fmt="4bit", qt="nf4", cs=True, xexp=BF16_RANGE, bad="x"),
    # an f32 (and an f16) dX over a 16-bit weight; non-finite rows; a poisoned weight block
    _d("grad", "dense 256x128", M=4, N=128, K=72, dt="bf16", xdt="f32", **_B4),
    _d("grad", "dense 128x128", M=5, N=192, K=72, dt="bf16", xdt="f16", fmt="int8", bad="x"),
    _d("grad", "dense 256x128", M=5, N=128, K=72, dt="f16", xdt="f32", fmt="fp8", bad="w", xexp=F16_RANGE),
    # through the ABI: dY aligned | 2 bytes off; the dense format (SwitchBack's dX); W off its alignment
    _d("grad_abi", "dense 256x128", M=4, N=128, K=72, dt="bf16", fmt="int8"),
    _g("grad_abi", "int8", "bf16", "bf16", M=4, N=128, K=72, off={"dy": 2}),
    _g("grad_abi", "int8", "bf16", "bf16", M=4, N=128, K=72, off={"w": 4}),
    _d("grad_abi", "dense 256x128", M=4, N=128, K=72, dt="f16", fmt="dense"),
    _g("grad_abi", "dense", "f16", "f16", M=4, N=128, K=72, off={"w": 8}),
    _g("grad_abi", "dense", "f16", "f16", M=4, N=128, K=76),
    _d("grad_abi", "dense 256x128", M=4, N=128, K=72, dt="f16", **_B4),
    _d("grad_abi", "dense 256x128", M=4, N=128, K=72, dt="f16", off={"w": 4}, **_B4),      # 4 bytes off 16: legal
    _g("grad_abi", "nf4", "f16", "f16", M=4, N=128, K=72, off={"w": 2}),
    _g("grad_abi", "nf4", "f16", "f16", M=4, N=128, K=72, off={"w": 1}),
    # the workspace: exact (above), NULL, 256 bytes short of the transposed weight, 16 bytes off 256
    _g("grad_abi", "int8", "bf16", "bf16", M=4, N=128, K=72, ws="null"),
    _g("grad_abi", "int8", "bf16", "bf16", M=4, N=128, K=72, ws="short"),
    _g("grad_abi", "int8", "bf16", "bf16", M=4, N=128, K=72, off={"ws": 16}),
]
# the smallest shape the plan splits, found with the restated plan (M = 1 ... 300 and K = 8 ... 520 over N in steps of 64): 36 k-steps in five
# slices of 8, 8, 8, 8 and 4; at 35 steps the 128 x 128 tiles stay unsplit.  And the same call with the transposed weight's bytes alone:
# one slice, bit-equal to a one-slice GEMM of the same product
SPLIT = dict(M=1, N=2304, K=8)
DENSE += [
    _d("grad_abi", "dense 256x128 x5", split=True, dt="bf16", **_B4, **SPLIT),
    _d("grad_abi", "dense 256x128", dt="bf16", ws="nosplit", **_B4, **SPLIT),
    _d("grad", "dense 256x128 x5", split=True, dt="f16", xdt="f32", fmt="int8", **SPLIT),
    _d("grad_abi", "dense 128x128", M=1, N=2240, K=8, dt="bf16", **_B4),               # 35 k-steps: not split
]

# ------------------------------------------------------------------------------------------------ the launch grid
# 65535 | 65536 row groups of k_grad_generic: past grid.y a workgroup walks on by the grid's height
GRID = [
    _g("grad", "nf4", "f32", "f32", M=262140, N=8, K=8),
    _g("grad", "nf4", "f32", "f32", M=262144, N=8, K=8),
    _g("grad", "fp4", "bf16", "bf16", M=262140, N=8, K=8, bs=16),
    _g("grad", "fp4", "f16", "f16", M=262144, N=8, K=8, bs=16, bias=True),
]

CASES = GRAD_T + GENERIC + DENSE + GRID


def derived(c):
    M = c.get("M", 0)
    return dict(M=M, groups=(M + GRAD_GM - 1) // GRAD_GM, slices=gemm_dense_plan(M, c["K"], c["N"])[1] if c["op"] != "grad_t" and grad_dense_shape(c) else 1,
                is16=c["dt"] != "f32", plain=not c.get("off") and not c.get("ws"))


# ------------------------------------------------------------------------------------------------ the closures' tables
# per kernel, the type axes and the values each takes in the sources (the switch arms and template arguments of grad_kernels.hip, read
# by tests/test_grad_forms_host.py); every value is taken by some case
FORMATS = ("nf4", "fp4", "int8", "fp8", "dense")
INSTANTIATED = {
    "k_dequant_t": dict(T=("f16", "bf16"), FMT=FORMATS, NESTED=(False, True)),
    "k_grad_generic": dict(T=DTS, O=DTS, FMT=FORMATS, NESTED=(False, True)),
}


def instantiations(kernel):
    """Every (axis values) tuple the kernel is compiled for: NESTED only with the 4-bit formats."""
    ax = INSTANTIATED[kernel]
    out = set()
    for T in ax["T"]:
        for O in ax.get("O", (None,)):
            for f in ax["FMT"]:
                for n in ax["NESTED"]:
                    if not n or f in ("nf4", "fp4"):
                        out.add((T, O, f, n))
    return out


def instantiation(c):
    """(kernel, (T, O, FMT, NESTED)) of the decode kernel the case runs (the pass of the dense path included); None where refused."""
    name = c["kernel"]
    if name == _NO:
        return None
    if name == _G:
        return "k_grad_generic", (c["dt"], c.get("xdt", c["dt"]), fmt_word(c), nested(c))
    return "k_dequant_t", (c["dt"], None, fmt_word(c), nested(c))


# what the scan of set_kernel_variant expands and no call reaches: the nested word behind a format without an absmax
UNREACHABLE = {f"grad_t {f} {t} nested {v}" for f in ("int8", "fp8", "dense") for t in ("f16", "bf16") for v in ("vec", "scalar")} | \
              {f"grad_generic {f} {t}>{o} nested" for f in ("int8", "fp8", "dense") for t in DTS for o in DTS}

_fullcall = ("grad", "grad_abi")
THRESHOLDS = [
    ("dense N >= 128", _fullcall, lambda c, d: c["N"] == 64 and d["is16"] and d["plain"] and c["kernel"] == _G,
     lambda c, d: c["N"] == 128 and d["plain"] and c["kernel"] == _D),
    ("dense N % 64", _fullcall, lambda c, d: c["N"] == 160 and d["is16"] and d["plain"] and c["kernel"] == _G and c["K"] == 72,
     lambda c, d: c["N"] == 192 and c["kernel"] == _D),
    ("dense blocksize 16 | 32", _fullcall, lambda c, d: c.get("bs") == 16 and c["N"] == 128 and c["kernel"] == _G,
     lambda c, d: c.get("bs") == 32 and c["N"] == 128 and c["kernel"] == _D),
    ("pass blocksize 4 | 8", ("grad_t",), lambda c, d: c.get("bs") == 4 and c["kernel"] == _NO, lambda c, d: c.get("bs") == 8 and c["kernel"] == _T),
    ("K % 8, 8-bit and dense formats", _fullcall, lambda c, d: c["K"] == 72 and c["fmt"] != "4bit" and d["plain"] and c["kernel"] == _D,
     lambda c, d: c["K"] == 76 and c["fmt"] != "4bit" and c["N"] == 128 and c["kernel"] == _G),
    ("pass K % 8, 8-bit and dense formats", ("grad_t",), lambda c, d: c["K"] == 72 and c["fmt"] != "4bit" and c["kernel"] == _T,
     lambda c, d: c["K"] == 76 and c["fmt"] != "4bit" and c["kernel"] == _NO),
    ("pass stores N % 8", ("grad_t",), lambda c, d: c["N"] % 8 == 0 and c["variant"].endswith("vec"),
     lambda c, d: c["N"] % 8 != 0 and c["variant"].endswith("scalar")),
    ("split-K of the dense path", _fullcall, lambda c, d: d["slices"] == 1 and c["N"] == 2240 and c["kernel"] == _D,
     lambda c, d: d["slices"] > 1 and c["kernel"] == _DS),
    ("split-K partials fit the workspace", ("grad_abi",), lambda c, d: d["slices"] > 1 and c.get("ws") == "nosplit" and c["kernel"] == _D,
     lambda c, d: d["slices"] > 1 and "ws" not in c and c["kernel"] == _DS),
    ("k_grad_generic: 65535 row groups in grid.y, f32", ("grad",), lambda c, d: d["groups"] == 65535 and not d["is16"], lambda c, d: d["groups"] == 65536 and not d["is16"]),
    ("k_grad_generic: 65535 row groups in grid.y, 16 bit", ("grad",), lambda c, d: d["groups"] == 65535 and d["is16"], lambda c, d: d["groups"] == 65536 and d["is16"]),
]

# every literal tests.forms.limit_counts finds on the host side of grad_kernels.hip -> its THRESHOLDS row(s), or ("no case", why)
_NOCASE = "no case"
LIMIT_CLAIMS = {
    "% 8": ["K % 8, 8-bit and dense formats", "pass K % 8, 8-bit and dense formats", "pass stores N % 8"],
    "% 64": "dense N % 64",
    "128": "dense N >= 128",
    "8": "pass blocksize 4 | 8",
    "32": "dense blocksize 16 | 32",
    "1": ["split-K of the dense path", "split-K partials fit the workspace"],
    "65535": ["k_grad_generic: 65535 row groups in grid.y, f32", "k_grad_generic: 65535 row groups in grid.y, 16 bit",
              (_NOCASE, "(K + 255) / 256 > 65535, the grid of the pass: a weight row of 16 M elements")],
    "1 << 31": (_NOCASE, "256 N 2 < 2^31, the pitch of the transposed weight: N of 2^22 and more"),
    "0x7FFFFFFF": (_NOCASE, "2^31 - 1 workgroups along n (the pass) or k (the generic kernel): a dimension of 2^37 and more"),
    "4": (_NOCASE, "sizeof(T) == 4 picks the dtype word of the variant: held by INSTANTIATED"),
}
# how often the host side compares with each literal: a new comparison changes a count until its THRESHOLDS row and cases follow
LIMIT_COUNTS = {"% 8": 4, "% 64": 1, "65535": 2, "0x7FFFFFFF": 2, "8": 2, "128": 1, "1 << 31": 1, "1": 3, "4": 2, "32": 1}
# the pointer tests of launch_dequant_t (the output) and linear_grad_input_dispatch (W by format, the workspace, dY), by their masks in source
# order; each is an operand of `off` with a case on both sides (OPERAND_ALIGNMENT_TESTED)
ALIGNMENT_MASKS = [15, 15, 3, 7, 255, 15]
OPERAND_ALIGNMENT_TESTED = {("grad_abi", "w"), ("grad_abi", "ws"), ("grad_abi", "dy"), ("grad_t", "w"), ("grad_t", "out")}
# offset and the form stays: dX of the generic kernel (no pointer test: 2-byte stores)
OPERAND_ALIGNMENT_FREE = {("grad_abi", "dx")}


def case_id(c):
    opts = "-".join(f"{k}{'' if v is True else v}" for k, v in sorted(c.items())
                    if k not in ("op", "kernel", "variant", "M", "N", "K", "off") and v not in (None, False))
    offs = "".join(f"-{k}+{v}" for k, v in sorted(c.get("off", {}).items()))
    return f"{c['op']}[{c['kernel']}]{c.get('M', '')}x{c['N']}x{c['K']}-{opts}{offs}".replace(" ", "")
