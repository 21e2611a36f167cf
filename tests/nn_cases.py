"""
The forms and limits of csrc/nn_kernels.hip, one table: k_embedding_4bit, k_embedding_8bit, k_quantize_rowwise_masked,
k_quantize_rowwise_masked_regs and k_outlier_add.  Data and host arithmetic only, importable without a GPU.

  op       embedding_4bit | embedding_8bit   functional.embedding_*: operands built directly (random bytes, random absmax / scales)
           outlier_linear                    functional.outlier_linear (its own `out` and `ws`, placed by the plan of tests/guard.py)
           outlier_abi                       mbnb_outlier_linear through ctypes: the only way to choose the workspace
  dt       the output dtype of a lookup, the compute dtype of the linear
  dim bs qt   a lookup's row width, blocksize and code table (every table has NUM rows)
  idx      the indices of a lookup: "many" (40 with repeats in a 5 x 8 tensor, row 0 and the last row among them), "one", "i32",
           "pad" (padding_idx set and looked up), "oob" (-1, num and 2^40 among valid rows)
  M N K n_out bias   the linear's shape, number of outlier columns and bias
  oob      True: the entries -1 and K mixed into the outlier indices (they contribute nothing on any path)
  off      {operand: bytes}: that operand starts so many bytes off its alignment -- packed / w / out of a lookup, x / ow / out / ws of the linear
  ws       the workspace of outlier_abi: "exact" (what mbnb_outlier_linear_workspace_bytes(M, K, n_out) asks for), "n0" (the n = 0 query),
           "two" (the first two regions only), "short" (one byte less than those)
  err      the text of the MBNB_ERR_ARG the call must answer with; nothing is written then

model(case) restates the launchers' conditions.  tests/test_gpu_nn_forms.py runs every case on guarded buffers under both fills;
tests/test_nn_forms_host.py closes the table over the source.
"""
from tests.gemm_variant_cases import tiles256

DTS = ("f16", "bf16", "f32")
ESIZE = {"f16": 2, "bf16": 2, "f32": 4}
EMB_OPS = ("embedding_4bit", "embedding_8bit")
LIN_OPS = ("outlier_linear", "outlier_abi")
OPERANDS = {"embedding_4bit": ("packed", "out"), "embedding_8bit": ("w", "out"), "outlier_linear": ("x", "ow", "out", "ws"),
            "outlier_abi": ("x", "ow", "out", "ws")}
PLAN_OPERANDS = {"embedding_4bit": ("out",), "embedding_8bit": ("out",), "outlier_linear": ("out", "ws"), "outlier_abi": ()}
REGS_MAX_K = 8192               # k_quantize_rowwise_masked_regs: four 16-byte pieces per thread of 256
MASK_MAX_BYTES = 65536          # the LDS column mask, K rounded up to 8
NUM = 11                        # rows of every lookup table


def offset(c, operand):
    return c.get("off", {}).get(operand, 0)


def is_emb(c):
    return c["op"] in EMB_OPS


# ------------------------------------------------------------------------------------------------ the launchers, restated
def ldx(n_out):
    return (n_out + 15) // 16 * 16


def _up(n):
    return (n + 255) & ~255


def layout_bytes(M, K, n_out):
    """outlier_linear_workspace_bytes: [x_q int8 M*K | pad to 256][x_scales f32 M | pad to 256][xo 16-bit M x ldx | pad to 256]."""
    return _up(M * K) + _up(4 * M) + _up(2 * ldx(n_out) * M)


def ws_query(M, K, n_out):
    """mbnb_outlier_linear_workspace_bytes: room for one chunk of 16 at the least."""
    return layout_bytes(M, K, max(n_out, 16))


def regions(M, K, n_out):
    """(off_s, off_x, end_x): where the scales begin, where xo begins, where xo's M x ldx values end."""
    off_s = _up(M * K)
    off_x = off_s + _up(4 * M)
    return off_s, off_x, off_x + 2 * ldx(n_out) * M


def ws_bytes(c):
    """What the call hands the library."""
    M, K, n = c["M"], c["K"], n_entries(c)
    mode = c.get("ws")
    if mode == "n0":
        return ws_query(M, K, 0)
    if mode == "two":
        return layout_bytes(M, K, 0)
    if mode == "short":
        return layout_bytes(M, K, 0) - 1
    return ws_query(M, K, n)            # "exact", and functional.py's own


def n_entries(c):
    """The length of the index list the library is given: n_out, plus the two out-of-range entries."""
    return c["n_out"] + (2 if c.get("oob") else 0)


def model(c):
    """Embeddings: (form, threads).  The linear: (quantiser, xo, epilogue, kernel, variant), epilogue "fused", "none" or
    ("add", vec_out, ow_vec); ("error", text) where the call is refused."""
    if is_emb(c):
        dim = c["dim"]
        src = offset(c, "packed") % 4 == 0 if c["op"] == "embedding_4bit" else offset(c, "w") % 8 == 0
        vec = dim % 8 == 0 and src and offset(c, "out") % 16 == 0
        return ("vec" if vec else "scalar"), (256 if dim >= 2048 else (128 if dim >= 1024 else 64))
    M, N, K, n, dt = c["M"], c["N"], c["K"], n_entries(c), c["dt"]
    is16 = dt != "f32"
    if ws_bytes(c) < layout_bytes(M, K, 0):
        return "error", "too small"
    if (K + 7) // 8 * 8 > MASK_MAX_BYTES:
        return "error", "too large for the LDS column mask"
    vec = K % 8 == 0 and offset(c, "x") % 16 == 0
    quant = "regs" if is16 and vec and K <= REGS_MAX_K else ("two_pass_vec" if vec else "two_pass_scalar")
    xo = n > 0 and ws_bytes(c) >= layout_bytes(M, K, n) and is16
    ep = (n == 0 or xo) and (n > 0 or bool(c.get("bias")))
    big = tiles256(M, N) >= 96
    fused = False
    if K % 16 != 0 or offset(c, "ws") % 16 != 0:
        kernel, variant = "i8_generic", ""
    elif ep and K % 128 == 0 and K >= 256 and 256 * K < 1 << 31 and big and is16 and (n == 0 or ldx(n) <= 64):
        kernel, variant, fused = "i8_dense+outliers", "i8_dense OUTL%d NCH%d" % (1 if dt == "f16" else 2, 2 if n > 0 and ldx(n) > 32 else 1), True
    elif K % 128 == 0 and big:
        kernel, variant, fused = "i8_mfma256", "", ep and is16
    else:
        kernel, variant = "i8_mfma128", ""
    if fused:
        epi = "fused"
    elif n > 0 or c.get("bias"):
        epi = ("add", N % 2 == 0 and offset(c, "out") % 8 == 0, n % 8 == 0 and offset(c, "ow") % 16 == 0)
    else:
        epi = "none"
    return quant, xo, epi, kernel, variant


def positions(c):
    """The case's outlier columns, unsorted: 1 and 0 (one dword, both halves), K - 1, the pair 11 | 10 (another group of 8), the first
    column of the scalar tail when K % 8 != 0, then columns 7 i + 13 (mod K) until there are n_out."""
    K, n_out = c["K"], c["n_out"]
    assert n_out <= K - 2, "two kept columns at the least"
    want = [1, 0, K - 1, 11, 10] + ([K // 8 * 8] if K % 8 else [])
    out = []
    for p in want + [(7 * i + 13) % K for i in range(4 * K)]:
        if len(out) == n_out:
            break
        if 0 <= p < K and p not in out and not (len(out) == n_out - 1 and len(set(range(K)) - set(out) - {p}) < 2):
            out.append(p)
    assert len(out) == n_out
    return out


def index_list(c):
    """What the library is given as outlier_indices: positions(c), with -1 and K mixed in for an `oob` case."""
    p = positions(c)
    if c.get("oob"):
        p = p[:1] + [-1] + p[1:] + [c["K"]]
    return p


# ------------------------------------------------------------------------------------------------ the cases
def _e4(dim, bs=64, qt="nf4", dt="f16", idx="many", **kw):
    return dict(op="embedding_4bit", dim=dim, bs=bs, qt=qt, dt=dt, idx=idx, **kw)


def _e8(dim, dt="f16", idx="many", **kw):
    return dict(op="embedding_8bit", dim=dim, dt=dt, idx=idx, **kw)


EMBEDDING = []
for _qt in ("nf4", "fp4"):                       # both code tables x the three output types, vector and scalar form
    for _dt in DTS:
        EMBEDDING += [_e4(72, 64, _qt, _dt), _e4(70, 64, _qt, _dt)]
for _dt in DTS:
    EMBEDDING += [_e8(72, _dt), _e8(70, _dt)]
EMBEDDING += [
    # the thread classes from both sides, a second trip of the vector loop for the low threads only, the smallest rows
    _e4(1016), _e4(1024, dt="bf16"), _e4(2040, qt="fp4"), _e4(2048), _e4(2056, dt="bf16"), _e4(4104, dt="f32"), _e4(8), _e4(2, bs=8),
    _e8(1016), _e8(1024, "bf16"), _e8(2040), _e8(2048, "f32"), _e8(2056), _e8(4104, "bf16"), _e8(8), _e8(2),
    # more columns than threads on the scalar path; odd widths of the 8-bit table
    _e4(100, dt="bf16"), _e4(100, qt="fp4", dt="f32"), _e8(100, "bf16"), _e8(13), _e8(65, "f32"), _e8(13, "bf16"),
    # blocksizes: 8; 20 and 36 (blocks straddle a group of 8); larger than the row; a ragged last block
    _e4(72, bs=8), _e4(72, bs=20, dt="bf16"), _e4(72, bs=36, qt="fp4"), _e4(72, bs=36, dt="f32"), _e4(72, bs=128), _e4(100, bs=36),
    # odd blocksizes: the two nibbles of a byte in different blocks (with an even blocksize a byte never straddles two)
    _e4(72, bs=9), _e4(72, bs=21, qt="fp4", dt="bf16"), _e4(70, bs=9, dt="f32"),
    # each pointer condition on its own (against 72 above)
    _e4(72, off={"packed": 1}), _e4(72, off={"packed": 2}), _e4(72, off={"out": 2}), _e4(72, off={"out": 4}), _e4(72, off={"out": 8}),
    _e4(72, dt="f32", off={"out": 4}), _e4(72, dt="f32", off={"out": 8}),
    _e8(72, off={"w": 4}), _e8(72, off={"out": 2}), _e8(72, off={"out": 4}), _e8(72, off={"out": 8}), _e8(72, "f32", off={"out": 8}),
    # indices
    _e4(72, idx="one"), _e4(72, idx="i32"), _e4(72, idx="pad"), _e4(72, idx="oob"), _e4(70, idx="oob", dt="bf16"), _e4(70, idx="pad"),
    _e8(72, idx="one"), _e8(72, idx="i32"), _e8(72, idx="pad"), _e8(72, idx="oob"), _e8(13, idx="oob"), _e8(70, idx="pad", dt="bf16"),
]


def _l(M, N, K, dt, n_out, bias=False, op="outlier_linear", **kw):
    return dict(op=op, M=M, N=N, K=K, dt=dt, n_out=n_out, bias=bias, **kw)


def _a(M, N, K, dt, n_out, bias=False, **kw):
    return _l(M, N, K, dt, n_out, bias, op="outlier_abi", **kw)


LINEAR = []
for _dt in DTS:                                   # every quantiser form x dtype: K = 200 | 203, and x two bytes off
    LINEAR += [_l(5, 6, 200, _dt, 5, True), _l(5, 6, 203, _dt, 5), _l(5, 6, 200, _dt, 5, True, off={"x": 2 if _dt != "f32" else 4})]
LINEAR += [
    # K: one group of 8, three, the second register slot, the register limit from both sides
    _l(5, 6, 8, "f16", 3, True), _l(5, 6, 24, "bf16", 5), _l(4, 6, 2056, "f16", 5, True), _l(4, 6, 2056, "f32", 5),
    _l(4, 6, 8192, "bf16", 5, True), _l(4, 6, 8200, "f16", 5, True), _l(4, 6, 8200, "bf16", 5),
    # the LDS mask limit from both sides
    _a(2, 8, MASK_MAX_BYTES, "f16", 2, True, ws="exact"), _a(2, 8, MASK_MAX_BYTES + 8, "f16", 2, True, ws="exact", err="too large for the LDS column mask"),
    _a(2, 8, MASK_MAX_BYTES + 8, "f32", 2, ws="exact", err="too large for the LDS column mask"),
    # M: one row, the row group of k_outlier_add from both sides, three groups
    _l(1, 6, 200, "f16", 5, True), _l(16, 6, 200, "bf16", 5, True), _l(17, 6, 200, "bf16", 5, True), _l(33, 6, 200, "f16", 5), _l(33, 6, 200, "f32", 5, True),
    # N: 2; odd (scalar accesses to out); a second workgroup in grid.x
    _l(5, 2, 200, "f16", 5, True), _l(5, 7, 200, "bf16", 5, True), _l(5, 7, 200, "f32", 5), _l(5, 512, 200, "f16", 5, True), _l(5, 514, 200, "bf16", 5, True),
    _l(5, 514, 200, "f32", 5, True),
    # out four bytes off 8 with N even
    _l(5, 6, 200, "f16", 5, True, off={"out": 4}), _l(5, 6, 200, "f32", 5, True, off={"out": 4}),
    # n_out: none with and without a bias; one; a full chunk; a ragged second chunk; a full and a scalar chunk; three chunks
    _l(5, 6, 200, "f16", 0, True), _l(5, 6, 200, "bf16", 0), _l(5, 6, 200, "f32", 0), _l(5, 6, 200, "f32", 0, True), _l(5, 6, 200, "bf16", 1, True),
    _l(5, 6, 200, "f16", 16, True), _l(5, 6, 200, "bf16", 17), _l(5, 6, 200, "f16", 24, True), _l(5, 6, 200, "bf16", 33, True), _l(5, 6, 200, "f32", 16),
    # the outlier weights two bytes off 16 at n_out = 16
    _l(5, 6, 200, "f16", 16, True, off={"ow": 2}),
    # a full chunk on the 16-byte weight loads in bf16, and under scalar accesses to out
    _l(5, 6, 200, "bf16", 16), _l(5, 7, 200, "f16", 16),
    # the int8 MFMA kernel (K % 16 == 0) under the add launch
    _l(17, 7, 208, "f16", 5, True), _l(5, 6, 208, "bf16", 0),
    # the workspace through the C ABI
    _a(17, 6, 200, "f16", 17, True, ws="exact"), _a(17, 6, 200, "f16", 17, True, ws="n0"), _a(5, 6, 200, "bf16", 5, ws="two"),
    _a(5, 6, 200, "bf16", 5, ws="short", err="too small"), _a(5, 6, 200, "f16", 5, True, ws="exact"), _a(5, 6, 200, "f16", 5, True, ws="exact", off={"ws": 16}),
    _l(5, 6, 200, "f16", 5, True, off={"ws": 16}),
    # the fused epilogue at the smallest shape the GEMM table uses for it
    _l(1536, 4096, 256, "f16", 32, True), _l(1536, 4096, 256, "bf16", 40),
    # entries -1 and K among the indices: nothing on the add path and nothing on the fused one
    _l(5, 6, 200, "f16", 5, True, oob=True), _l(5, 6, 200, "f32", 5, oob=True),
]

CASES = EMBEDDING + LINEAR


def derived(c):
    if is_emb(c):
        form, threads = model(c)
        return dict(form=form, threads=threads, plain=not c.get("off") and c["idx"] == "many")
    m = model(c)
    d = dict(groups=(c["M"] + 15) // 16, wgs=(c["N"] + 511) // 512, is16=c["dt"] != "f32", plain=not c.get("off") and not c.get("ws") and not c.get("oob"),
             error=m[0] == "error")
    if not d["error"]:
        d.update(quant=m[0], xo=m[1], epi=m[2], kernel=m[3], add=m[2] not in ("fused", "none"))
    return d


def case_id(c):
    offs = "".join(f"-{k}+{v}" for k, v in sorted(c.get("off", {}).items()))
    if is_emb(c):
        bs = f"-{c['qt']}-bs{c['bs']}" if c["op"] == "embedding_4bit" else ""
        return f"{c['op']}-{c['dim']}-{c['dt']}{bs}-{c['idx']}{offs}"
    opts = "".join(f"-{k}" + ("" if c[k] is True else str(c[k])) for k in ("bias", "oob", "ws") if c.get(k))
    return f"{c['op']}-{c['M']}x{c['N']}x{c['K']}-{c['dt']}-n{c['n_out']}{opts}{offs}" + ("-err" if "err" in c else "")


# ------------------------------------------------------------------------------------------------ the closures' tables
def _ok(d):
    return not d["error"]


THRESHOLDS = [
    ("embedding threads: dim 1016 | 1024", EMB_OPS, lambda c, d: c["dim"] == 1016 and d["threads"] == 64, lambda c, d: c["dim"] == 1024 and d["threads"] == 128),
    ("embedding threads: dim 2040 | 2048", EMB_OPS, lambda c, d: c["dim"] == 2040 and d["threads"] == 128, lambda c, d: c["dim"] == 2048 and d["threads"] == 256),
    ("embedding dim % 8", EMB_OPS, lambda c, d: c["dim"] == 72 and d["plain"] and d["form"] == "vec", lambda c, d: c["dim"] == 70 and d["form"] == "scalar"),
    ("quantiser K % 8", ("outlier_linear",), lambda c, d: c["K"] == 200 and d["plain"] and d["quant"] in ("regs", "two_pass_vec"),
     lambda c, d: c["K"] == 203 and d["quant"] == "two_pass_scalar"),
    ("quantiser in registers up to K = 8192", ("outlier_linear",), lambda c, d: c["K"] == 8192 and d["quant"] == "regs", lambda c, d: c["K"] == 8200 and d["quant"] == "two_pass_vec"),
    ("the LDS column mask", ("outlier_abi",), lambda c, d: (c["K"] + 7) // 8 * 8 == MASK_MAX_BYTES and _ok(d), lambda c, d: (c["K"] + 7) // 8 * 8 == MASK_MAX_BYTES + 8 and d["error"]),
    ("xo for 16-bit types only", ("outlier_linear",), lambda c, d: d["is16"] and c["n_out"] > 0 and d["plain"] and d["xo"], lambda c, d: not d["is16"] and c["n_out"] > 0 and not d["xo"]),
    ("xo when the workspace has room", ("outlier_abi",), lambda c, d: c.get("ws") == "exact" and c["n_out"] == 17 and d["xo"], lambda c, d: c.get("ws") == "n0" and c["n_out"] == 17 and not d["xo"]),
    ("the first two regions of the workspace", ("outlier_abi",), lambda c, d: c.get("ws") == "two" and _ok(d) and not d["xo"], lambda c, d: c.get("ws") == "short" and d["error"]),
    ("k_outlier_add: rows 16 | 17", ("outlier_linear",), lambda c, d: c["M"] == 16 and d["add"] and d["groups"] == 1, lambda c, d: c["M"] == 17 and d["add"] and d["groups"] == 2),
    ("k_outlier_add: columns 512 | 514", ("outlier_linear",), lambda c, d: c["N"] == 512 and d["add"] and d["wgs"] == 1, lambda c, d: c["N"] == 514 and d["add"] and d["wgs"] == 2),
    ("k_outlier_add: N % 2", ("outlier_linear",), lambda c, d: c["N"] == 6 and d["plain"] and d["add"] and d["epi"][1], lambda c, d: c["N"] == 7 and d["add"] and not d["epi"][1]),
    ("k_outlier_add: n_out % 8", ("outlier_linear",), lambda c, d: c["n_out"] == 16 and d["plain"] and d["add"] and d["epi"][2], lambda c, d: c["n_out"] == 17 and d["add"] and not d["epi"][2]),
    ("no launch after the GEMM without outliers and bias", ("outlier_linear",), lambda c, d: c["n_out"] == 0 and c["bias"] and d["add"], lambda c, d: c["n_out"] == 0 and not c["bias"] and d["epi"] == "none"),
    ("the fused epilogue", ("outlier_linear",), lambda c, d: _ok(d) and d["epi"] == "fused" and d["xo"], lambda c, d: _ok(d) and d["add"] and d["xo"]),
]

# every literal tests.forms.limit_counts finds in the launchers of nn_kernels.hip -> its THRESHOLDS row(s), or ("no case", why)
_NOCASE = "no case"
LIMIT_CLAIMS = {
    "% 8": ["embedding dim % 8", "quantiser K % 8", "k_outlier_add: n_out % 8"],
    "% 2": "k_outlier_add: N % 2",
    "1024": "embedding threads: dim 1016 | 1024",
    "2048": "embedding threads: dim 2040 | 2048",
    "8192": "quantiser in registers up to K = 8192",
    str(MASK_MAX_BYTES): "the LDS column mask",
    "2": "xo for 16-bit types only",
    "65535": (_NOCASE, "65535 row groups of k_outlier_add in grid.y: M of 2^20, held by tests/gemm_variant_cases.py's pair of cases"),
}
LIMIT_COUNTS = {"% 8": 4, "% 2": 1, "1024": 2, "2048": 2, "8192": 1, str(MASK_MAX_BYTES): 1, "2": 2, "65535": 1}
# the pointer tests of the three launchers by their masks, in source order: packed, out; W, out; X, out, ow
ALIGNMENT_MASKS = [3, 15, 7, 15, 15, 7, 15]
# (op, operand) -> (the aligned call's form, the form with that operand alone off its alignment); each has a pair of cases
ALIGNMENT_TESTED = {
    ("embedding_4bit", "packed"): ("vec", "scalar"), ("embedding_4bit", "out"): ("vec", "scalar"),
    ("embedding_8bit", "w"): ("vec", "scalar"), ("embedding_8bit", "out"): ("vec", "scalar"),
    ("outlier_linear", "x"): ("regs", "two_pass_scalar"), ("outlier_linear", "out"): (True, False), ("outlier_linear", "ow"): (True, False),
}
# offset and the form stays: the workspace 16 bytes off its 256-byte alignment
ALIGNMENT_FREE = {("outlier_linear", "ws"), ("outlier_abi", "ws")}


def form_of(c, operand):
    """The part of model(c) the operand's pointer test decides."""
    m = model(c)
    if is_emb(c) or operand in ("x", "ws"):
        return m[0]
    return m[2][1 if operand == "out" else 2]


def pairs(op, operand):
    """Cases of `op` offset in `operand` alone, each with the case that differs from it by that offset only."""
    out = []
    for c in CASES:
        if c["op"] == op and set(c.get("off", {})) == {operand}:
            out += [(c, b) for b in CASES if "off" not in b and {k: v for k, v in c.items() if k != "off"} == b]
    return out
