"""
One table of the VARIANTS of the GEMM-family launchers: which template instantiation or runtime branch a call takes behind its
kernel name (mbnb_last_kernel's second string, _native.last_variant()).  Cases in the format of tests/kernel_cases.py plus

  variant  the variant the case must report ("" where its launcher sets none)
  bs2      a nested absmax (cs) re-quantised at this second blocksize instead of 256 (96: not a power of two)
  view     besides "rows" and "misaligned" (the activation): one other operand off its alignment, a slice of a larger buffer --
           "absmax+4" (the f32 absmax 4 bytes off 16), "codes+1" (the nested int8 absmax codes 1 byte off 4), "packed+4" / "packed+2"
           (the packed nibbles off 16 / off 4), "w+1" (the int8 / FP8 weight), "a+1" / "b+1" (matmul_int8's operands)
  M > 65535 cases are the launch-grid cases: a row index that no longer fits grid.y

Data and host arithmetic only, importable without a GPU.  tests/test_gpu_elementwise.py runs every case through the runners of
the kernel-name table (every output element against float64 on poisoned allocations, the name AND the variant checked after a
sentinel launch); tests/test_gemm_variants_host.py closes the table over the sources: every variant csrc/ can report has a case,
model_variant(c) -- the launchers' conditions and the plan functions restated below -- gives each case's variant, and the
INSTANTIATED, THRESHOLDS and ALIGNMENT_TESTED tables hold.  The GPU test holds the same `variant` key against the library, so
the restatement is itself checked on the GPU.
"""
from tests.kernel_cases import BF16_RANGE, F16_RANGE, _c, case_id  # noqa: F401


# ------------------------------------------------------------------------------------------------ the plans, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def padded(K, bs):
    kp = _cdiv(K, bs) * bs
    return kp + bs if kp % 2 else kp


def tiles256(M, N):
    return _cdiv(M, 256) * _cdiv(N, 256)


def matmul4_splitk_slices(M, N, K):                                   # matmul4_kernels.hip
    if M <= 4 or K % 64 != 0:
        return 1
    if tiles256(M, N) >= 96:
        return 1
    tiles = _cdiv(M, 128) * _cdiv(N, 128)
    s = min(_cdiv(512, tiles), K // 256, 16)
    return 1 if s < 2 else s


def _small_shape_up_to(M, N, K, Kw, max_m, min_m):                    # gemm_small.hip
    return ((M > min_m or (M > 16 and N * K > 1 << 24)) and M <= max_m and K % 256 == 0 and K >= 512 and K <= 16 * 2048 and
            Kw % 256 == 0 and N >= 64 and 256 * K * 2 < 1 << 31)


def gemm_small_shape(M, N, K, Kw):
    return _small_shape_up_to(M, N, K, Kw, 512, 28)


def gemm_small8_shape(M, N, K):
    return _small_shape_up_to(M, N, K, K, 384, 32)


def gemm_small_plan(M, N, K, maxs_mf8=16):
    """(nf, slices, us, mf) of gemm_small.hip's cost model, the same double arithmetic in the same order."""
    steps = K // 256
    best, best_t = (1, 1, 1e30, 8 if M > 64 else 4), 1e30
    mf_lo = 8 if M > 64 and (M > 256 or maxs_mf8 != 16) else 4
    mf_hi = 8 if M > 64 else 4
    for mf in range(mf_lo, mf_hi + 1, 4):
        mt = _cdiv(M, 16 * mf)
        nf_max = 2 if M > 256 and maxs_mf8 == 16 else 1
        for nf in range(1, nf_max + 1):
            wgs = _cdiv(N, 64 * nf) * mt
            maxs = maxs_mf8 if mf == 8 else (16 if M > 64 else 8)
            step_us = 3.0 if nf == 2 else (1.6 if M > 256 else 0.4 + float(mf * 8) / 55.0)
            for s in range(1, min(16, steps) + 1):
                per = _cdiv(steps, s)
                if per > maxs:
                    continue
                split_fixed = 5.0 if M > 256 else (4.5 if mf_lo != mf_hi else 2.0)
                t = float((wgs * s + 255) // 256) * (2.5 + float(per) * step_us) + \
                    ((8.0 * float(s) * float(M) * float(N) / 6.0e6 + split_fixed) if s > 1 else 0.0)
                if t < best_t - 1e-9:
                    best_t, best = t, (nf, s, t, mf)
    return best


def gemm_dense_shape(M, N, K, Kw):                                    # gemm_dense.hip
    if K % 64 != 0 or K < 128 or Kw % 8 != 0:
        return False
    if 256 * max(K, Kw) * 2 >= 1 << 31 or M * N * 4 >= 1 << 40:
        return False
    return (M >= 256 and M * N >= 1500000) or (M > 256 and M * N >= 1000000)


def gemm_dense_plan(M, N, K):
    """(fm, slices): 8 = 256 x 256 tiles, 4 = 256 (n) x 128 (m), 2 = 128 x 128."""
    tn = _cdiv(N, 256)
    tiles8, tiles4 = _cdiv(M, 256) * tn, _cdiv(M, 128) * tn
    tiles2 = _cdiv(M, 128) * _cdiv(N, 128)
    steps = K // 64
    best, best_t = (8, 1), 1e30
    if K >= 192 and tiles8 < 96:
        rounds = (tiles2 + 255) // 256
        best_t = float(rounds) * float(steps) * (0.36 if tiles2 <= 128 else 0.47)
        best = (2, 1)
    for fm in (8, 4):
        tiles = tiles8 if fm == 8 else tiles4
        step = 1.3 if fm == 8 else 0.75
        for s in range(1, 9):
            per = _cdiv(steps, s)
            if s > 1 and (per < 8 or tiles8 >= 96):
                break
            rounds = (tiles * s + 255) // 256
            t = float(rounds) * float(per) * step + ((6.0 + 8.0 * float(s) * float(M) * float(N) / 6.0e6) if s > 1 else 0.0)
            if t < best_t * (1.0 if fm == 8 else 0.97):
                best_t, best = t, (fm, s)
    return best


def _nb_tile_cost(fn, nk):
    fixed, step = (6.5, 7.0, 7.5, 7.9), (0.85, 1.008, 1.18, 1.30)
    return fixed[fn - 5] + float(nk) * step[fn - 5]


def _nb_makespan(na, ca, nb, cb):
    P = 256
    qa, ra = divmod(na, P)
    lo = float(qa) * ca
    hi = lo + ca
    n_lo, n_hi = P - ra, ra
    end = 0.0 if na == 0 else (hi if ra else lo)
    while nb > 0:
        use_lo = n_hi == 0 or lo <= hi
        cap = n_lo if use_lo else n_hi
        if use_lo:
            lo += cb
            t = lo
        else:
            hi += cb
            t = hi
        end = max(end, t)
        nb -= min(nb, cap)
    return end


def gemm_dense_nb_plan(M, N, K, fm=8):
    """(fna, cols_a, cols_b): the column-balanced grid, (8, c8, 0) where uniform 256-wide columns stay."""
    tiles_m, U, nk = _cdiv(M, 256), _cdiv(N, 32), K // 64
    c8 = _cdiv(U, 8)
    tiles8 = tiles_m * c8
    f = float(tiles8 % 256) / 256.0
    cost8 = _nb_tile_cost(8, nk)
    uniform_t = cost8 * (float(tiles8 // 256) + ((0.3 + 0.7 * f if 0.3 + 0.7 * f > 0.66 else 0.66) if f > 0.0 else 0.0))
    if fm == 4:
        tiles4 = _cdiv(M, 128) * c8
        uniform_t = float((tiles4 + 255) // 256) * (5.0 + 0.75 * float(nk))
    best = (8, c8, 0, uniform_t)
    if tiles8 <= 256 or f == 0.0 or tiles_m > 256 or c8 > 1 << 20:
        return best[:3]
    span = 256 // tiles_m + 1
    for fna in (8, 7, 6):
        fnb = fna - 1
        cmin, cmax = _cdiv(U, fna), _cdiv(U, fnb)
        C = cmin
        while C <= cmax and C <= cmin + span:
            a = max(U - fnb * C, 0)
            if a <= C:
                t = _nb_makespan(tiles_m * a, _nb_tile_cost(fna, nk), tiles_m * (C - a), _nb_tile_cost(fnb, nk)) * \
                    (1.02 if 0 < a < C else 1.0)
                if t < best[3]:
                    best = (fna, a, C - a, t)
            C += 1
    if best[3] > 0.96 * uniform_t:
        return (8, c8, 0)
    return best[:3]


def dense_variant(M, N, K, fm, slices):
    """launch_gemm_dense: what the plan's (fm, slices) -- or a forced tile, fm 9 / 10 -- runs."""
    if fm == 2:
        return "dense 128x128"
    if fm in (8, 4) and slices <= 1:
        fna, _, cols_b = gemm_dense_nb_plan(M, N, K, fm)
        if cols_b > 0 or fna != 8:
            return f"dense_nb {fna}/{fna - 1}"
    tile = "dense 256x128" if fm in (4, 10) else "dense 256x256"
    if slices <= 1:
        return tile
    kps = _cdiv(K // 64, slices) * 64
    return f"{tile} x{_cdiv(K, kps)}"


def gemm_small_one_round(M, N, K, Kw):
    if M <= 256 or not gemm_small_shape(M, N, K, Kw):
        return False
    nf, slices, us, _ = gemm_small_plan(M, N, K)
    if _cdiv(N, 64 * nf) * _cdiv(M, 128) * slices > 256:
        return False
    tiles2 = _cdiv(M, 128) * _cdiv(N, 128)
    boundary = 0.6 if N * Kw <= 1 << 25 else 3.6
    dense_us = float(N) * float(Kw) * 2.53 / 4.4e6 + boundary + \
        float((tiles2 + 255) // 256) * float(K // 64) * (0.36 if tiles2 <= 128 else 0.47) + 2.0
    return us < dense_us * 1.05


def gemm_mid_shape(M, N, K):                                          # gemm_mid.hip
    return 32 < M <= (384 if N >= 8192 else 192) and tiles256(M, N) < 96 and K % 64 == 0 and K >= 256


def gemm_mid_slices(M, N, K):
    tiles = _cdiv(M, 128) * _cdiv(N, 64)
    if tiles >= 256:
        return 1
    s = min(_cdiv(256, tiles), K // 256, 8)
    return 1 if s < 2 else s


def gemm_f32_shape(M, N, K, Kw):                                      # gemm_f32.hip
    if M < 5 or N < 32 or K < 16 or K % 4 != 0 or Kw % 4 != 0:
        return False
    r = float(N) * float(K) / 16777216.0
    return float((M + 7) // 8) * (0.15 + 17.0 * r) + 4.0 > 18.0 + 31.0 * r


def gemm_f32_plan(M, N, K):
    if _cdiv(M, 128) * _cdiv(N, 128) >= 256:
        return 128, 1
    t64 = _cdiv(M, 64) * _cdiv(N, 64)
    s = max(min(_cdiv(1024, t64), K // 256, 16), 1)
    kps = _cdiv(_cdiv(K, s), 32) * 32                                 # GF_BK = 32
    return 64, _cdiv(K, kps)


# ------------------------------------------------------------------------------------------------ the launchers, restated
def derived(c):
    """The quantities the launchers branch on.  Workspaces are what functional.py allocates (the library's own query), pointers
    are 16-byte aligned unless the case's `view` says otherwise."""
    M = c["M"] if "M" in c else 1
    for v in c.get("lead", ()):
        M = M * v if "M" not in c else M
    N, K = c["N"], c["K"]
    if c["op"] == "matmul_int8":
        return dict(M=M, N=N, K=K, tiles256=tiles256(M, N), NK=N * K, dt=None, out=c["out"], nested=False, fused=False,
                    a_aligned=c.get("view") != "a+1", b_aligned=c.get("view") != "b+1")
    bs = c.get("bs", 64)
    Kw = padded(K, bs) if c["op"] == "matmul_4bit" else c.get("ldw", K)
    return dict(M=M, N=N, K=K, bs=bs, Kw=Kw, ku=_cdiv(K, 2048), tiles256=tiles256(M, N), NK=N * K, x_aligned=c.get("view") != "misaligned", am_aligned=c.get("view") != "absmax+4",
                codes_aligned=c.get("view") != "codes+1", packed16=c.get("view") not in ("packed+4", "packed+2"), packed4=c.get("view") != "packed+2",
                w_aligned=c.get("view") != "w+1",
                dt=c.get("dt"), out=c.get("out", c.get("dt")), nested=bool(c.get("cs")), bs2=c.get("bs2", 256), fused=bool(c.get("fused")))


def _matmul4(c, d):
    M, N, K, Kw, bs, al = d["M"], d["N"], d["K"], d["Kw"], d["bs"], d["x_aligned"]
    is16 = d["dt"] != "f32"
    nested, bs2 = d["nested"], d["bs2"]
    bs2_pow2 = bs2 & (bs2 - 1) == 0
    fast_layout = is16 and bs >= 32 and Kw % 32 == 0 and K % 8 == 0 and al and d["packed16"]
    codes_ok = not nested or d["codes_aligned"]                          # (am.i8 & 3) == 0 where a kernel reads the codes by dwords
    small_first = fast_layout and gemm_small_one_round(M, N, K, Kw)
    if not d["fused"] and not small_first:
        if is16 and gemm_dense_shape(M, N, K, Kw) and al and d["packed4"]:
            fm, s = gemm_dense_plan(M, N, K)
            return ("dequant+dense_splitk" if s > 1 else "dequant+dense"), dense_variant(M, N, K, fm, s)
        if not is16 and gemm_f32_shape(M, N, K, Kw) and al:
            bt, s = gemm_f32_plan(M, N, K)
            return ("dequant+dense_f32_splitk" if s > 1 else "dequant+dense_f32"), ("f32 128" if bt == 128 else f"f32 64 x{s}")
    if is16:
        slices = matmul4_splitk_slices(M, N, K)
        splitk = fast_layout and slices > 1
        small_ok = bs >= 32 and gemm_small_shape(M, N, K, Kw)
        skinny = fast_layout and M >= 2 and not small_ok and (M <= 32 or (M <= 64 and N * K <= 1 << 24)) and K % 128 == 0
        if fast_layout and M <= 16 and K % 32 == 0 and not (splitk and M > 4) and not skinny:
            xlds = 8 * ((K + 2047) & ~2047) * 2 <= 65536
            if d["out"] == d["dt"]:
                ku = _cdiv(K, 2048)
                if M == 1 and bs == 64 and Kw == K and K % 64 == 0 and K >= 1024 and ku <= 8 and \
                        (not nested or (bs2_pow2 and d["codes_aligned"] and (K // 64) % 4 == 0)):
                    KU = ku if ku <= 4 else (6 if ku <= 6 else 8)
                    return "gemv", f"gemv_lean ku{ku}/KU{KU}"
            if M == 1:
                t = (1, 2, 2) if N >= 8192 else (1, 1, 2)
            elif not xlds:
                t = (2, 1, 2) if M == 2 else ((4, 2, 1) if M <= 4 else (8, 1, 1))
            else:
                t = (2, 1, 2) if M == 2 else ((4, 1, 2) if M <= 4 else (8, 1, 2))
            return "gemv", "gemv MT%d NR%d KU%d %s" % (t + ("lds" if xlds else "regs",))
        if skinny:
            return "skinny_mfma16", "skinny MT%d NR1" % (1 if M <= 16 else (2 if M <= 32 else 4))
        if fast_layout and small_ok:
            nf, s, _, mf = gemm_small_plan(M, N, K)
            steps = K // 256
            per = _cdiv(steps, s)
            used = _cdiv(steps, per)
            if M <= 64:
                v = (4, 1, 0)
            elif mf == 4:
                v = (4, 1, 16)
            elif nf == 2:
                v = (8, 2, 16)
            else:
                v = (8, 1, 16) if per > 8 else (8, 1, 0)
            return ("mfma_small_splitk" if used > 1 else "mfma_small"), "small MF%d NF%d S%d x%d" % (v + (used,))
        if fast_layout and bs == 64 and Kw % 256 == 0 and gemm_mid_shape(M, N, K) and (not nested or (bs2 >= 4 and bs2_pow2 and codes_ok)):
            s = gemm_mid_slices(M, N, K)
            kps = _cdiv(_cdiv(K, 256), s) * 256
            s = _cdiv(K, kps)
            return ("mfma_mid_splitk", f"mid x{s}") if s > 1 else ("mfma_mid", "mid")
        if fast_layout and K % 64 == 0 and tiles256(M, N) >= 96:
            if not nested or bs2_pow2:
                am4 = bs == 64 and Kw % 256 == 0 and (not nested or (bs2 >= 4 and codes_ok))
                if am4 and K >= 128 and 256 * K * 2 < 1 << 31 and (nested or d["am_aligned"]):   # gemm_fused4_shape, its f32 absmax 16-byte aligned
                    return "mfma256f", "fused4"
                return "mfma256", "gemm256p am4" if am4 else "gemm256p"
            return "mfma256", "gemm256"
        if fast_layout:
            if splitk:
                return "mfma128_splitk", f"decode128 x{slices}"
            return "mfma128", "decode128"
    flags = (1 if Kw % 8 == 0 and bs >= 8 and d["packed4"] else 0) | (2 if al and (K * (2 if is16 else 4)) % 16 == 0 else 0)
    return "generic", "generic ROWS%d flags%d" % (1 if M == 1 else (4 if M <= 4 else 8), flags)


def _linear8(c, d):
    M, N, K, al = d["M"], d["N"], d["K"], d["x_aligned"]
    pre = "w8a16_" if c["op"] == "linear_int8" else "fp8a16_"
    is16 = d["dt"] != "f32"
    ws = M > 16                                                          # functional.py asks for a workspace from 17 rows
    if not d["fused"] and is16 and ws and gemm_dense_shape(M, N, K, K) and al:
        fm, s = gemm_dense_plan(M, N, K)
        return pre + ("dequant+dense_splitk" if s > 1 else "dequant+dense"), dense_variant(M, N, K, fm, s)
    if is16:
        wal = al and d["w_aligned"]
        if 32 < M <= 256 and gemm_small8_shape(M, N, K) and wal:
            s = gemm_small_plan(M, N, K, 8)[1]
            steps = K // 256
            used = _cdiv(steps, _cdiv(steps, s))
            return pre + ("small_splitk" if used > 1 else "small"), "small8 MF%d x%d" % (4 if M <= 64 else 8, used)
        if 1 <= M <= 64 and K % 128 == 0 and wal:
            return pre + "skinny", "skinny8 MT%d" % (1 if M <= 16 else (2 if M <= 32 else 4))
        fast = K % 16 == 0 and wal and M > 4
        if fast and K % 64 == 0 and tiles256(M, N) >= 96:
            return pre + "mfma256", "gemm256w"
        if fast:
            s = matmul4_splitk_slices(M, N, K)
            if s > 1 and ws:
                return pre + "mfma128_splitk", f"decode128 x{s}"
            return pre + "mfma128", "decode128"
    return pre + "generic", "linear8_generic"


def _dense(c, d):
    M, N, K = d["M"], d["N"], d["K"]
    if c["op"] == "linear_dense":
        fm, s = gemm_dense_plan(M, N, K)
    else:
        tile, s = c["tile"], c["slices"]
        fm = {1: 10, 2: 9, 3: 2}[tile] if tile else gemm_dense_plan(M, N, K)[0]
        if s == 0:
            s = gemm_dense_plan(M, N, K)[1]
    v = dense_variant(M, N, K, fm, s)
    name = v if " x" not in v else v.split(" x")[0] + "_splitk"
    return (name if not v.startswith("dense_nb") else "dense_nb "), v


def _outlier(c, d):
    M, N, K, n_out = d["M"], d["N"], d["K"], c["n_out"]
    if K % 16 != 0:
        return "i8_generic", ""
    ldx = _cdiv(n_out, 16) * 16
    big = tiles256(M, N) >= 96
    if K % 128 == 0 and K >= 256 and 256 * K < 1 << 31 and big and d["dt"] != "f32" and (n_out == 0 or ldx <= 64) and (n_out > 0 or c.get("bias")):
        return "i8_dense+outliers", "i8_dense OUTL%d NCH%d" % (1 if d["dt"] == "f16" else 2, 2 if n_out > 0 and ldx > 32 else 1)
    if K % 128 == 0 and big:
        return "i8_mfma256", ""
    return "i8_mfma128", ""


def _matmul_int8(c, d):
    M, N, K = d["M"], d["N"], d["K"]
    big = tiles256(M, N) >= 96
    inplace_shape = K % 128 == 0 and K >= 256 and N % 16 == 0 and N >= 256 and big and 256 * K < 1 << 31 and K * N < (1 << 31) - (1 << 17)
    ab = d["a_aligned"] and d["b_aligned"]
    if inplace_shape and ab:
        return "i8_inplace4", ""
    dense = K % 128 == 0 and K >= 256 and 256 * K < 1 << 31 and big and N % 64 == 0
    direct_shape = K % 128 == 0 and N % 16 == 0 and big
    ws = not inplace_shape and (dense or not direct_shape)               # matmul_int8_workspace_bytes: N * K bytes, or none
    if ws and dense and ab:
        return "i8_transpose+dense", "i8_dense"
    if direct_shape and ab:
        return "i8_mfma256", ""
    if K % 16 != 0 or not ws or not d["a_aligned"]:
        return "i8_generic", ""
    return ("i8_mfma256", "") if K % 128 == 0 and big else ("i8_mfma128", "")


def model(c):
    """(kernel name, variant) the launchers' conditions give the case."""
    d = derived(c)
    op = c["op"]
    if op == "matmul_4bit":
        return _matmul4(c, d)
    if op in ("linear_int8", "matmul_fp8"):
        return _linear8(c, d)
    if op in ("linear_dense", "gemm_dense"):
        return _dense(c, d)
    if op == "outlier_linear":
        return _outlier(c, d)
    if op == "matmul_int8":
        return _matmul_int8(c, d)
    raise KeyError(op)


def model_variant(c):
    return model(c)[1]


# ------------------------------------------------------------------------------------------------ the cases
def _v(op, kernel, variant, **kw):
    return _c(op, kernel, variant=variant, **kw)


_M4 = "matmul_4bit"

GEMV = [
    # k_gemv4_lean<KU>: M = 1, blocksize 64, 1024 <= K <= 16384; ku = ceil(K / 2048) runs on KU = ku up to 4, then 6 and 8 -- ku 5 and 7
    # with a whole chunk past K
    _v(_M4, "gemv", "gemv_lean ku1/KU1", M=1, N=260, K=1024, dt="f16", bias=True),               # the shortest K of the lean form
    _v(_M4, "gemv", "gemv MT1 NR1 KU2 lds", M=1, N=260, K=960, dt="f16"),                       # ... and the longest it refuses below
    _v(_M4, "gemv", "gemv_lean ku2/KU2", M=1, N=130, K=2112, dt="bf16", qt="fp4"),
    _v(_M4, "gemv", "gemv MT1 NR1 KU2 lds", M=1, N=130, K=2112, dt="bf16", cs=True),            # nested: (K / 64) % 4 != 0 keeps it off the lean form
    _v(_M4, "gemv", "gemv_lean ku3/KU3", M=1, N=131, K=4160, dt="f16", bad="x"),
    _v(_M4, "gemv", "gemv_lean ku4/KU4", M=1, N=67, K=6208, dt="bf16", bias=True, xexp=BF16_RANGE),
    _v(_M4, "gemv", "gemv_lean ku5/KU6", M=1, N=133, K=8256, dt="f16", xexp=F16_RANGE),            # chunk 6 wholly past K
    _v(_M4, "gemv", "gemv_lean ku6/KU6", M=1, N=65, K=12288, dt="bf16", cs=True),
    _v(_M4, "gemv", "gemv_lean ku7/KU8", M=1, N=129, K=14336, dt="bf16", bias=True, bad="w"),    # a real layer width; chunk 8 wholly past K
    _v(_M4, "gemv", "gemv_lean ku8/KU8", M=1, N=70, K=16384, dt="f16", cs=True, qt="fp4"),        # the longest K of the lean form
    _v(_M4, "gemv", "gemv MT1 NR1 KU2 regs", M=1, N=70, K=16448, dt="f16"),                      # ... and the first it refuses
    # k_gemv4<MT, NR, KU, XLDS>: the activations staged in LDS up to K = 4096, in registers beyond
    _v(_M4, "gemv", "gemv MT1 NR1 KU2 lds", M=1, N=100, K=4096, dt="f16", out="f32"),           # the longest K in LDS (not lean: the output dtype differs)
    _v(_M4, "gemv", "gemv MT1 NR2 KU2 lds", M=1, N=8192, K=512, dt="bf16", bias=True),
    _v(_M4, "gemv", "gemv MT1 NR1 KU2 lds", M=1, N=8191, K=512, dt="bf16", bias=True),
    _v(_M4, "gemv", "gemv MT1 NR2 KU2 regs", M=1, N=8193, K=4160, dt="f16", out="bf16"),
    _v(_M4, "gemv", "gemv MT2 NR1 KU2 lds", M=2, N=66, K=4064, dt="f16", qt="fp4", cs=True),
    _v(_M4, "gemv", "gemv MT2 NR1 KU2 regs", M=2, N=66, K=4128, dt="bf16", out="f32"),
    _v(_M4, "gemv", "gemv MT4 NR1 KU2 lds", M=3, N=70, K=4064, dt="bf16", bias=True),
    _v(_M4, "gemv", "gemv MT4 NR1 KU2 lds", M=4, N=70, K=4064, dt="f16", out="f32"),
    _v(_M4, "gemv", "gemv MT4 NR2 KU1 regs", M=4, N=70, K=4128, dt="f16", bias=True),
    _v(_M4, "gemv", "gemv MT8 NR1 KU2 lds", M=5, N=70, K=4064, dt="f16", xexp=F16_RANGE),
    _v(_M4, "gemv", "gemv MT8 NR1 KU2 lds", M=16, N=70, K=4064, dt="bf16", bs=128),
    _v(_M4, "gemv", "gemv MT8 NR1 KU1 regs", M=9, N=70, K=4128, dt="bf16", bias=True),
    _v(_M4, "gemv", "gemv MT8 NR1 KU1 regs", M=16, N=67, K=4128, dt="f16"),
    _v(_M4, "mfma128", "decode128", M=17, N=70, K=4064, dt="bf16"),                              # 17 rows: off the GEMV
]

SKINNY = [
    _v(_M4, "skinny_mfma16", "skinny MT1 NR1", M=16, N=50, K=384, dt="bf16", bias=True),
    _v(_M4, "skinny_mfma16", "skinny MT1 NR1", M=2, N=50, K=4096, dt="f16"),                     # K % 128 == 0: the skinny kernel, not k_gemv4
    _v(_M4, "skinny_mfma16", "skinny MT2 NR1", M=17, N=50, K=384, dt="f16", out="bf16"),
    _v(_M4, "skinny_mfma16", "skinny MT2 NR1", M=32, N=50, K=640, dt="bf16", cs=True),
    _v(_M4, "skinny_mfma16", "skinny MT4 NR1", M=33, N=50, K=384, dt="f16", qt="fp4"),
    _v(_M4, "skinny_mfma16", "skinny MT4 NR1", M=64, N=43690, K=384, dt="bf16", bias=True),       # N * K just below 2^24
    _v(_M4, "mfma256", "gemm256p", M=64, N=43691, K=384, dt="bf16", bias=True),                  # ... and just above: not skinny from 33 rows
    _v(_M4, "mfma128", "decode128", M=65, N=50, K=384, dt="f16"),                                # 65 rows: off the skinny kernel
    _v(_M4, "skinny_mfma16", "skinny MT2 NR1", M=28, N=64, K=512, dt="f16"),                     # k_gemm_small takes K % 256 == 0 from 29 rows ...
    _v(_M4, "mfma_small", "small MF4 NF1 S0 x1", M=29, N=64, K=512, dt="f16"),
    _v(_M4, "skinny_mfma16", "skinny MT2 NR1", M=17, N=4096, K=4096, dt="bf16"),                 # ... and from 17 on more than 2^24 weights
    _v(_M4, "mfma_small_splitk", "small MF4 NF1 S0 x3", M=17, N=4097, K=4096, dt="bf16"),
]

SMALL = [
    # k_gemm_small<MF, NF, MAXS>: the plan of gemm_small_plan (the smallest shapes the cost model sends to each)
    _v(_M4, "mfma_small", "small MF4 NF1 S0 x1", M=64, N=70, K=768, dt="bf16", bias=True, fused=True),
    _v(_M4, "mfma_small_splitk", "small MF4 NF1 S0 x5", M=33, N=64, K=1280, dt="f16", fused=True, out="f32"),
    _v(_M4, "mfma_small", "small MF4 NF1 S16 x1", M=65, N=70, K=768, dt="f16", fused=True, qt="fp4"),
    _v(_M4, "mfma_small_splitk", "small MF4 NF1 S16 x5", M=130, N=700, K=2304, dt="bf16", fused=True, cs=True),      # 2 + 2 + 2 + 2 + 1 steps
    _v(_M4, "mfma_small", "small MF8 NF1 S0 x1", M=257, N=70, K=768, dt="bf16", fused=True, bias=True, cs=True),
    _v(_M4, "mfma_small_splitk", "small MF8 NF1 S0 x5", M=512, N=70, K=1280, dt="f16", fused=True, bad="x"),
    _v(_M4, "mfma_small", "small MF8 NF1 S16 x1", M=257, N=2048, K=2304, dt="f16", fused=True),
    _v(_M4, "mfma_small_splitk", "small MF8 NF1 S16 x2", M=129, N=4096, K=4352, dt="bf16", fused=True),     # 9 + 8 steps
    _v(_M4, "mfma_small", "small MF8 NF2 S16 x1", M=257, N=8192, K=512, dt="bf16", fused=True, bias=True),
    _v(_M4, "mfma_small_splitk", "small MF8 NF2 S16 x5", M=257, N=2048, K=4352, dt="f16", fused=True),      # 4 + 4 + 4 + 4 + 1 steps
    _v(_M4, "mfma_small", "small MF8 NF1 S0 x1", M=300, N=512, K=1024, dt="f16"),                            # 257-512 rows in one round stay fused
    _v(_M4, "mfma128_splitk", "decode128 x3", M=513, N=70, K=768, dt="bf16", fused=True),                   # 513 rows: off k_gemm_small
]

MID = [
    _v(_M4, "mfma_mid", "mid", M=65, N=48, K=256, dt="f16", bias=True, cs=True),
    _v(_M4, "mfma_mid_splitk", "mid x3", M=192, N=48, K=768, dt="f16", qt="fp4"),
    _v(_M4, "mfma_mid_splitk", "mid x5", M=150, N=40, K=2304, dt="f16", out="f32", bias=True),             # 9 blocks: 2 + 2 + 2 + 2 + 1
    _v(_M4, "mfma128_splitk", "decode128 x3", M=193, N=48, K=768, dt="bf16", cs=True),
]

DECODE = [
    _v(_M4, "mfma128", "decode128", M=5, N=70, K=72, dt="bf16", bias=True),
    _v(_M4, "mfma128_splitk", "decode128 x5", M=200, N=300, K=1344, dt="f16", bias=True, fused=True),       # 21 steps: 5 + 5 + 5 + 5 + 1
    # 95 and 96 tiles of 256 x 256
    _v(_M4, "mfma128", "decode128", M=1280, N=4864, K=128, dt="f16", fused=True),
    _v(_M4, "mfma256", "gemm256p", M=1536, N=4096, K=128, dt="f16", fused=True),                          # K_weight % 256 != 0: no AM4
    _v(_M4, "mfma256f", "fused4", M=1536, N=4096, K=256, dt="bf16", fused=True, bias=True),
    _v(_M4, "mfma256f", "fused4", M=1281, N=4865, K=256, dt="f16", fused=True, cs=True, out="f32"),
    _v(_M4, "mfma256", "gemm256p am4", M=1537, N=4000, K=256, dt="f16", fused=True, view="absmax+4"),      # fused4 needs a 16-byte aligned absmax
    _v(_M4, "mfma256", "gemm256", M=1537, N=4000, K=192, dt="bf16", fused=True, cs=True, bs2=96, bias=True),   # blocksize2 no power of two
]

DENSE4 = [
    # every dense tile and every column-balanced pair through a public op, the plan's own choice
    _v(_M4, "dequant+dense", "dense 128x128", M=1024, N=1000, K=192, dt="f16", bias=True),
    _v(_M4, "dequant+dense", "dense 256x128", M=1024, N=1000, K=128, dt="bf16"),
    _v(_M4, "dequant+dense", "dense 256x256", M=1025, N=21787, K=128, dt="f16", bias=True),
    _v(_M4, "dequant+dense", "dense_nb 6/5", M=769, N=18715, K=128, dt="bf16", bias=True),
    _v(_M4, "dequant+dense", "dense_nb 8/7", M=1537, N=23291, K=128, dt="f16"),
    _v(_M4, "dequant+dense_splitk", "dense 256x128 x4", M=300, N=5000, K=6080, dt="bf16", bias=True),       # 95 steps: 24 + 24 + 24 + 23
    _v(_M4, "dequant+dense", "dense 256x128", M=1280, N=4864, K=192, dt="f16"),                              # 95 tiles of 256 x 256 ...
    _v(_M4, "dequant+dense", "dense 256x128", M=1536, N=4096, K=192, dt="f16"),                              # ... and 96
    _v(_M4, "mfma_small", "small MF8 NF1 S0 x1", M=256, N=5859, K=512, dt="bf16"),                          # M * N just below 1.5 M: fused
    _v(_M4, "dequant+dense", "dense 128x128", M=256, N=5860, K=512, dt="bf16"),
    _v(_M4, "dequant+dense_f32", "f32 128", M=2048, N=2048, K=64, dt="f32", bias=True),
    _v(_M4, "dequant+dense_f32_splitk", "f32 64 x2", M=200, N=1000, K=520, dt="f32", out="f16"),
]

GENERIC = [_v(_M4, "generic", f"generic ROWS{rows} flags{fl}", M=M, N=67, **kw)
           for rows, M in ((1, 1), (4, 3), (8, 9))
           for fl, kw in ((0, dict(K=100, bs=4, dt="f16")), (1, dict(K=100, bs=64, dt="bf16", bias=True)),
                          (2, dict(K=96, bs=4, dt="bf16", qt="fp4")), (3, dict(K=128, bs=16, dt="f16", cs=True)))]
GENERIC += [
    _v(_M4, "generic", "generic ROWS4 flags3", M=4, N=67, K=72, dt="f32", out="f16"),
    _v(_M4, "generic", "generic ROWS8 flags3", M=5, N=67, K=72, dt="f32", bias=True),
    # the first pointer test of every dispatcher: an activation 2 bytes off 16-byte alignment takes the generic kernel
    _v(_M4, "generic", "generic ROWS1 flags1", M=1, N=130, K=2112, dt="bf16", view="misaligned"),           # aligned: gemv_lean ku2/KU2
    _v(_M4, "generic", "generic ROWS8 flags1", M=16, N=50, K=384, dt="bf16", view="misaligned"),            # aligned: skinny MT1 NR1
    _v(_M4, "generic", "generic ROWS8 flags1", M=1024, N=1000, K=128, dt="bf16", view="misaligned"),        # aligned: dense 256x128
]

# the launch grids: a row (group) index past what grid.y holds
GRID = [
    _v(_M4, "generic", "generic ROWS8 flags3", M=524280, N=8, K=72, dt="f16", bs=16),                       # 65535 groups of 8 rows
    _v(_M4, "generic", "generic ROWS8 flags3", M=524288, N=8, K=72, dt="f16", bs=16, bias=True),            # 65536
    _v("outlier_linear", "i8_generic", "", M=1048560, N=8, K=8, dt="f16", n_out=3, bias=True),              # k_outlier_add: 65535 groups of 16 rows
    _v("outlier_linear", "i8_generic", "", M=1048576, N=8, K=8, dt="bf16", n_out=3, bias=True),             # 65536
]

_W8 = [
    ("skinny", "skinny8 MT1", dict(M=1, N=50, K=128, dt="bf16")),
    ("skinny", "skinny8 MT1", dict(M=16, N=50, K=384, dt="f16", bias=True)),
    ("skinny", "skinny8 MT2", dict(M=17, N=50, K=384, dt="bf16")),
    ("skinny", "skinny8 MT2", dict(M=32, N=50, K=512, dt="f16", bias=True)),
    ("skinny", "skinny8 MT4", dict(M=64, N=50, K=384, dt="bf16", bias=True)),
    ("small", "small8 MF4 x1", dict(M=33, N=70, K=512, dt="f16")),
    ("small", "small8 MF4 x1", dict(M=64, N=70, K=768, dt="bf16", bias=True)),
    ("small", "small8 MF8 x1", dict(M=65, N=70, K=512, dt="f16", bias=True)),
    ("small_splitk", "small8 MF4 x5", dict(M=40, N=64, K=1280, dt="bf16")),
    ("small_splitk", "small8 MF8 x5", dict(M=256, N=70, K=1280, dt="f16", bias=True)),
    ("mfma128_splitk", "decode128 x5", dict(M=257, N=70, K=1280, dt="bf16", bias=True)),                     # 257 rows: off the small kernel
    ("mfma128", "decode128", dict(M=5, N=70, K=80, dt="bf16")),
    ("generic", "linear8_generic", dict(M=4, N=70, K=80, dt="bf16")),                                      # up to 4 rows
    ("generic", "linear8_generic", dict(M=3, N=67, K=64, dt="f32", bias=True)),
    ("mfma128", "decode128", dict(M=1280, N=4864, K=128, dt="f16", fused=True)),                            # 95 tiles of 256 x 256 ...
    ("mfma256", "gemm256w", dict(M=1536, N=4096, K=128, dt="f16", fused=True, bias=True)),                   # ... and 96
    ("dequant+dense", "dense 128x128", dict(M=1024, N=1000, K=192, dt="bf16")),
    ("dequant+dense", "dense 256x128", dict(M=1024, N=1000, K=128, dt="f16", bias=True)),
    ("dequant+dense", "dense 256x256", dict(M=513, N=13824, K=128, dt="bf16")),
    ("dequant+dense", "dense_nb 7/6", dict(M=769, N=22555, K=128, dt="f16", bias=True)),
    ("dequant+dense_splitk", "dense 256x128 x4", dict(M=300, N=5000, K=6080, dt="bf16")),
    # a misaligned activation: the generic kernel
    ("generic", "linear8_generic", dict(M=16, N=50, K=384, dt="f16", view="misaligned")),                   # aligned: skinny8 MT1
    ("generic", "linear8_generic", dict(M=64, N=70, K=768, dt="bf16", view="misaligned")),                  # aligned: small8 MF4 x1
    ("generic", "linear8_generic", dict(M=1024, N=1000, K=128, dt="f16", view="misaligned")),               # aligned: dense 256x128
    # the launch grid: one row per grid.y
    ("generic", "linear8_generic", dict(M=65535, N=8, K=64, dt="f32")),
    ("generic", "linear8_generic", dict(M=65536, N=8, K=64, dt="f32", bias=True)),
    ("generic", "linear8_generic", dict(M=65535, N=8, K=72, dt="f16", bias=True)),
    ("generic", "linear8_generic", dict(M=65536, N=8, K=72, dt="bf16")),
]
LINEAR8 = ([_v("linear_int8", "w8a16_" + k, v, **kw) for k, v, kw in _W8] + [_v("matmul_fp8", "fp8a16_" + k, v, **kw) for k, v, kw in _W8])

OUTLIER = [
    # k_gemm_dense<.., I8, OUTL, NCH>: f16 / bf16 rounding chain x one / two chunks of 32 outlier columns; 96 tiles of 256 x 256
    _v("outlier_linear", "i8_dense+outliers", "i8_dense OUTL1 NCH1", M=1536, N=4096, K=256, dt="f16", n_out=32, bias=True),
    _v("outlier_linear", "i8_dense+outliers", "i8_dense OUTL1 NCH2", M=1536, N=4096, K=256, dt="f16", n_out=33),
    _v("outlier_linear", "i8_dense+outliers", "i8_dense OUTL2 NCH1", M=1537, N=4000, K=256, dt="bf16", n_out=16, bias=True),
    _v("outlier_linear", "i8_dense+outliers", "i8_dense OUTL2 NCH2", M=1537, N=4000, K=384, dt="bf16", n_out=64, bias=True),
    _v("outlier_linear", "i8_dense+outliers", "i8_dense OUTL2 NCH2", M=1536, N=4096, K=256, dt="bf16", n_out=40, xexp=(0, 24)),   # rows past f16's range
    _v("outlier_linear", "i8_mfma256", "", M=1536, N=4096, K=256, dt="bf16", n_out=65, bias=True),             # 65 columns: past the epilogue's 64
    _v("outlier_linear", "i8_mfma128", "", M=1280, N=4864, K=256, dt="f16", n_out=33, bias=True),              # 95 tiles
]

DENSE_ABI = [
    # the split 256 x 256 tile is no plan's choice: forced through mbnb_gemm_dense's tile code
    _v("gemm_dense", "dense 256x256_splitk", "dense 256x256 x3", M=300, N=520, K=704, ldw=712, tile=2, slices=3, dt="f16", bias=True),   # 4 + 4 + 3 steps
    # matmul_int8 with B transposed into the workspace: k_gemm_dense<.., I8> without an epilogue (k_transpose_i8_64 / _128 before it)
    _v("matmul_int8", "i8_transpose+dense", "i8_dense", M=24321, N=64, K=256, out="f16"),
    _v("matmul_int8", "i8_transpose+dense", "i8_dense", M=24321, N=128, K=384, out="f32"),
]

LIMITS = [
    # k_gemm_mid up to 384 rows on wide layers (N >= 8192), and below 96 tiles of 256 x 256
    _v(_M4, "mfma_mid", "mid", M=384, N=8192, K=256, dt="f16", fused=True),
    _v(_M4, "mfma128", "decode128", M=385, N=8192, K=256, dt="f16", fused=True),
    _v(_M4, "mfma_mid", "mid", M=300, N=12032, K=256, dt="bf16", fused=True, bias=True),              # 94 tiles
    _v(_M4, "mfma256f", "fused4", M=300, N=12288, K=256, dt="bf16", fused=True, bias=True),           # 96
    # k_gemm_small: K up to 16 x 2048, N from 64
    _v(_M4, "mfma_small_splitk", "small MF4 NF1 S0 x16", M=64, N=64, K=32768, dt="bf16"),
    _v(_M4, "skinny_mfma16", "skinny MT4 NR1", M=64, N=64, K=33024, dt="bf16"),
    _v(_M4, "skinny_mfma16", "skinny MT4 NR1", M=64, N=63, K=768, dt="bf16", fused=True),
    # the dense path: K from 128, M * N from 10^6 above 256 rows; the dequantise pass's form up to 2^25 weights and, above, from 2048 rows
    _v(_M4, "mfma128", "decode128", M=1024, N=1000, K=64, dt="f16"),
    _v(_M4, "mfma128", "decode128", M=257, N=3891, K=128, dt="f16"),
    _v(_M4, "dequant+dense", "dense 256x128", M=257, N=3892, K=128, dt="f16"),
    _v(_M4, "dequant+dense", "dense 256x256", M=2048, N=8065, K=4160, dt="bf16"),                     # N * K just below 2^25
    _v(_M4, "dequant+dense", "dense 256x256", M=2048, N=8066, K=4160, dt="bf16", cs=True),            # ... just above, 2048 rows
    _v(_M4, "dequant+dense", "dense 256x256", M=2047, N=8066, K=4160, dt="f16"),                      # ... and 2047
    _v("linear_int8", "w8a16_dequant+dense", "dense 256x256", M=2048, N=8065, K=4160, dt="bf16"),
    _v("linear_int8", "w8a16_dequant+dense", "dense 256x256", M=2048, N=8066, K=4160, dt="bf16"),
    _v("linear_int8", "w8a16_dequant+dense", "dense 256x256", M=2047, N=8066, K=4160, dt="f16"),
    _v("matmul_fp8", "fp8a16_dequant+dense", "dense 256x256", M=2048, N=8066, K=4160, dt="bf16"),
    _v("matmul_fp8", "fp8a16_dequant+dense", "dense 256x256", M=2047, N=8066, K=4160, dt="f16"),
    # the f32 path: N from 32, K from 16 (the cost inequality lets M >= 752 in at this size)
    _v(_M4, "dequant+dense_f32", "f32 64 x1", M=800, N=32, K=16, dt="f32", bs=16),
    _v(_M4, "generic", "generic ROWS8 flags3", M=800, N=31, K=16, dt="f32", bs=16),
    _v(_M4, "generic", "generic ROWS8 flags3", M=800, N=32, K=12, dt="f32", bs=16),
    # outlier_linear's row quantiser: the row in registers up to K = 8192 (k_quantize_rowwise_masked_regs), the two-pass form beyond
    _v("outlier_linear", "i8_mfma128", "", M=64, N=96, K=8192, dt="f16", n_out=5, bias=True),
    _v("outlier_linear", "i8_mfma128", "", M=64, N=96, K=8208, dt="bf16", n_out=5),
]

ALIGN = [
    # one operand off its alignment, everything else as in an aligned case of the table
    _v(_M4, "generic", "generic ROWS8 flags3", M=16, N=50, K=384, dt="bf16", view="packed+4"),             # aligned16(packed); aligned: skinny MT1 NR1
    _v(_M4, "generic", "generic ROWS4 flags2", M=4, N=67, K=128, dt="f16", bs=16, view="packed+2"),        # flags bit 0; aligned: flags3
    _v(_M4, "generic", "generic ROWS8 flags2", M=1024, N=1000, K=128, dt="bf16", view="packed+2"),         # the dense path's packed & 3; aligned: dense 256x128
    _v(_M4, "gemv", "gemv MT1 NR1 KU2 regs", M=1, N=65, K=12288, dt="bf16", cs=True, view="codes+1"),      # aligned: gemv_lean ku6/KU6
    _v(_M4, "mfma128", "decode128", M=65, N=48, K=256, dt="f16", cs=True, view="codes+1"),                 # aligned: mid
    _v(_M4, "mfma256f", "fused4", M=1537, N=4000, K=256, dt="f16", cs=True, fused=True),
    _v(_M4, "mfma256", "gemm256p", M=1537, N=4000, K=256, dt="f16", cs=True, fused=True, view="codes+1"),  # neither fused4 nor AM4
    _v(_M4, "dequant+dense_f32", "f32 64 x1", M=300, N=1000, K=260, dt="f32"),
    _v(_M4, "generic", "generic ROWS8 flags1", M=300, N=1000, K=260, dt="f32", view="misaligned"),         # the f32 path's A; flags bit 1
    _v("matmul_int8", "i8_generic", "", M=24321, N=64, K=256, out="f16", view="a+1"),                     # aligned: i8_transpose+dense
    _v("matmul_int8", "i8_mfma256", "", M=24321, N=64, K=256, out="bf16", view="b+1"),                    # B through the generic transpose
    _v("matmul_int8", "i8_generic", "", M=2560, N=2560, K=256, out="bf16", view="b+1"),                   # aligned: i8_inplace4 (no workspace)
]
for _op, _pre in (("linear_int8", "w8a16_"), ("matmul_fp8", "fp8a16_")):
    ALIGN += [
        _v(_op, _pre + "generic", "linear8_generic", M=16, N=50, K=384, dt="f16", view="w+1"),             # aligned: skinny8 MT1
        _v(_op, _pre + "generic", "linear8_generic", M=64, N=70, K=768, dt="bf16", view="w+1"),            # aligned: small8 MF4 x1
        _v(_op, _pre + "generic", "linear8_generic", M=5, N=70, K=80, dt="bf16", view="w+1"),              # aligned: decode128
    ]

CASES = DENSE_ABI + LIMITS + ALIGN + GEMV + SKINNY + SMALL + MID + DECODE + DENSE4 + GENERIC + GRID + LINEAR8 + OUTLIER

# what the scan of the sources expands and no call can reach: MBNB_GEMV's `xlds ? "lds" : "regs"` under launch_matmul4's
# `else if (!xlds)` -- the register-light triples run only without LDS staging, the other two only with it
UNREACHABLE = {"gemv MT4 NR2 KU1 lds", "gemv MT8 NR1 KU1 lds", "gemv MT4 NR1 KU2 regs", "gemv MT8 NR1 KU2 regs"}


# ------------------------------------------------------------------------------------------------ the closures' tables
def axis_value(c, d, axis):
    return {"dt": d["dt"], "out": d["out"], "qt": c.get("qt", "nf4"), "cs": d["nested"]}[axis]


_16, _3, _QT, _CS = ("f16", "bf16"), ("f16", "bf16", "f32"), ("nf4", "fp4"), (False, True)
_FUSED4 = dict(dt=_16, out=_3, qt=_QT, cs=_CS)
# the type axes a launcher instantiates, per kernel name: every value is taken by some case of this table or of tests/kernel_cases.py
# (each axis on its own).  The W8A16 family's weight bytes (int8 / FP8) are in the name.
INSTANTIATED = {
    "gemv": _FUSED4, "skinny_mfma16": _FUSED4, "mfma_small": _FUSED4, "mfma_small_splitk": _FUSED4, "mfma_mid": dict(dt=_16, out=_16, cs=_CS),
    "mfma_mid_splitk": _FUSED4, "mfma128": dict(dt=_16), "mfma128_splitk": dict(dt=_16, out=_3, cs=_CS), "mfma256": _FUSED4,
    "mfma256f": dict(dt=_16, out=_3, cs=_CS), "dequant+dense": dict(dt=_16, cs=_CS), "dequant+dense_splitk": dict(dt=("bf16",)),
    "dequant+dense_f32": dict(dt=("f32",)), "dequant+dense_f32_splitk": dict(dt=("f32",), out=("f16", "f32")),
    "generic": dict(dt=_3, out=_3, qt=_QT, cs=_CS),
    "i8_dense+outliers": dict(dt=_16), "i8_mfma256": dict(dt=("bf16",)), "i8_mfma128": dict(dt=_16), "i8_generic": dict(dt=_16),
}
INSTANTIATED["dense 256x256_splitk"] = dict(dt=_16)
INSTANTIATED["i8_transpose+dense"] = dict(out=_3)
for _pre in ("w8a16_", "fp8a16_"):
    for _k in ("skinny", "small", "small_splitk", "mfma128", "mfma128_splitk", "dequant+dense"):
        INSTANTIATED[_pre + _k] = dict(dt=_16)
    INSTANTIATED[_pre + "mfma256"] = dict(dt=("f16",))
    INSTANTIATED[_pre + "dequant+dense_splitk"] = dict(dt=("bf16",))
    INSTANTIATED[_pre + "generic"] = dict(dt=_3)


def _is(variant_prefix):
    return lambda c, d: c["variant"].startswith(variant_prefix)


def _m(lo, hi=None, **cond):
    """A case with lo <= M (<= hi) whose derived values equal `cond`."""
    return lambda c, d: lo <= d["M"] <= (lo if hi is None else hi) and all(d[k] == v for k, v in cond.items())


_M4OPS, _W8OPS = ("matmul_4bit",), ("linear_int8", "matmul_fp8")
# (what, ops, a case on the first side, a case on the second side): every integer limit the GEMM launchers compare M, N, K or a tile
# count with, for each op that meets it
THRESHOLDS = [
    ("lean GEMV from K = 1024", _M4OPS, lambda c, d: d["M"] == 1 and d["K"] == 960, lambda c, d: d["K"] == 1024 and c["variant"] == "gemv_lean ku1/KU1"),
    ("lean GEMV up to K = 16384 (ku <= 8)", _M4OPS, lambda c, d: d["K"] == 16384 and c["variant"] == "gemv_lean ku8/KU8",
     lambda c, d: d["M"] == 1 and d["K"] == 16448),
    ("lean GEMV ku <= 4 on its own KU, ku 5 on KU = 6", _M4OPS, _is("gemv_lean ku4/KU4"), _is("gemv_lean ku5/KU6")),
    ("lean GEMV ku <= 6 on KU = 6, ku 7 on KU = 8", _M4OPS, _is("gemv_lean ku6/KU6"), _is("gemv_lean ku7/KU8")),
    ("k_gemv4 stages K <= 4096 in LDS, M = 1", _M4OPS, lambda c, d: d["M"] == 1 and d["K"] == 4096 and c["variant"].endswith("lds"),
     lambda c, d: d["M"] == 1 and d["K"] == 4160 and c["variant"].endswith("regs")),
    ("k_gemv4 stages K <= 4096 in LDS, 2 <= M <= 16", _M4OPS, lambda c, d: 2 <= d["M"] <= 16 and d["K"] == 4064 and c["variant"].endswith("lds"),
     lambda c, d: 2 <= d["M"] <= 16 and d["K"] == 4128 and c["variant"].endswith("regs")),
    ("k_gemv4 two rows per wave from N = 8192", _M4OPS, lambda c, d: d["N"] == 8191 and "NR1" in c["variant"], lambda c, d: d["N"] == 8192 and "NR2" in c["variant"]),
    ("k_gemv4 M = 1 | 2", _M4OPS, _is("gemv MT1"), _is("gemv MT2")),
    ("k_gemv4 M <= 4 | 5", _M4OPS, lambda c, d: d["M"] == 4 and c["variant"].startswith("gemv MT4"), lambda c, d: d["M"] == 5 and c["variant"].startswith("gemv MT8")),
    ("GEMV M <= 16 | 17", _M4OPS, lambda c, d: d["M"] == 16 and c["kernel"] == "gemv", lambda c, d: d["M"] == 17 and c["kernel"] == "mfma128"),
    ("skinny MT: M <= 16 | 17", _M4OPS + _W8OPS, lambda c, d: d["M"] == 16 and "skinny" in c["variant"] and "MT1" in c["variant"],
     lambda c, d: d["M"] == 17 and "skinny" in c["variant"] and "MT2" in c["variant"]),
    ("skinny MT: M <= 32 | 33", _M4OPS, lambda c, d: d["M"] == 32 and "MT2" in c["variant"], lambda c, d: d["M"] == 33 and "MT4" in c["variant"]),
    ("skinny up to M = 64", _M4OPS, lambda c, d: d["M"] == 64 and c["kernel"] == "skinny_mfma16", lambda c, d: d["M"] == 65 and c["kernel"] == "mfma128"),
    ("skinny at 33 <= M <= 64 up to N * K = 2^24", _M4OPS, lambda c, d: d["M"] == 64 and d["NK"] == (1 << 24) - 256 and c["kernel"] == "skinny_mfma16",
     lambda c, d: d["M"] == 64 and d["NK"] == (1 << 24) + 128 and c["kernel"] == "mfma256"),
    ("k_gemm_small from 29 rows", _M4OPS, lambda c, d: d["M"] == 28 and c["kernel"] == "skinny_mfma16", lambda c, d: d["M"] == 29 and c["kernel"] == "mfma_small"),
    ("k_gemm_small from 17 rows above 2^24 weights", _M4OPS, lambda c, d: d["M"] == 17 and d["NK"] == 1 << 24 and c["kernel"] == "skinny_mfma16",
     lambda c, d: d["M"] == 17 and d["NK"] == (1 << 24) + 4096 and c["kernel"] == "mfma_small_splitk"),
    ("k_gemm_small MF = 4 up to 64 rows", _M4OPS, lambda c, d: d["M"] == 64 and "MF4 NF1 S0" in c["variant"], lambda c, d: d["M"] == 65 and "MF4 NF1 S16" in c["variant"]),
    ("k_gemm_small MF = 8 from 257 rows", _M4OPS, lambda c, d: d["M"] == 256 and c["variant"].startswith("small"), lambda c, d: d["M"] == 257 and "MF8" in c["variant"]),
    ("k_gemm_small up to 512 rows", _M4OPS, lambda c, d: d["M"] == 512 and c["variant"].startswith("small"), lambda c, d: d["M"] == 513 and d["fused"]),
    ("k_gemm_small MAXS: more than 8 steps a slice", _M4OPS, _is("small MF8 NF1 S0"), _is("small MF8 NF1 S16")),
    ("k_gemm_mid up to 192 rows", _M4OPS, lambda c, d: d["M"] == 192 and c["variant"].startswith("mid"), lambda c, d: d["M"] == 193 and c["kernel"] == "mfma128_splitk"),
    ("96 tiles of 256 x 256, fused", _M4OPS + _W8OPS, lambda c, d: d["tiles256"] == 95 and d["fused"] and c["variant"] == "decode128",
     lambda c, d: d["tiles256"] == 96 and d["fused"] and c["variant"] in ("gemm256p", "fused4", "gemm256w")),
    ("96 tiles of 256 x 256, the dense plan", _M4OPS, lambda c, d: d["tiles256"] == 95 and c["kernel"] == "dequant+dense", lambda c, d: d["tiles256"] == 96 and c["kernel"] == "dequant+dense"),
    ("96 tiles of 256 x 256, the outlier epilogue", ("outlier_linear",), lambda c, d: d["tiles256"] == 95 and c["kernel"] == "i8_mfma128",
     lambda c, d: d["tiles256"] == 96 and c["kernel"] == "i8_dense+outliers"),
    ("64 outlier columns in the epilogue", ("outlier_linear",), lambda c, d: c["n_out"] == 64 and c["kernel"] == "i8_dense+outliers",
     lambda c, d: c["n_out"] == 65 and c["kernel"] == "i8_mfma256"),
    ("one chunk of 32 outlier columns", ("outlier_linear",), lambda c, d: c["n_out"] == 32 and "NCH1" in c["variant"], lambda c, d: c["n_out"] == 33 and "NCH2" in c["variant"]),
    ("the dense path from 256 rows and 1.5 M outputs", _M4OPS, lambda c, d: d["M"] == 256 and d["N"] == 5859 and "dense" not in c["kernel"],
     lambda c, d: d["M"] == 256 and d["N"] == 5860 and c["kernel"] == "dequant+dense"),
    ("generic ROWS: M = 1 | <= 4 | more", _M4OPS, _is("generic ROWS1"), _is("generic ROWS4")),
    ("generic ROWS: M <= 4 | 5", _M4OPS, lambda c, d: d["M"] == 4 and c["variant"].startswith("generic ROWS4"), lambda c, d: d["M"] == 5 and c["variant"].startswith("generic ROWS8")),
    ("generic: 65535 row groups in grid.y", _M4OPS, _m(524280), _m(524288)),
    ("W8A16 small from 33 rows", _W8OPS, lambda c, d: d["M"] == 32 and "skinny8" in c["variant"], lambda c, d: d["M"] == 33 and "small8" in c["variant"]),
    ("W8A16 small MF: M <= 64 | 65", _W8OPS, lambda c, d: d["M"] == 64 and "small8 MF4" in c["variant"], lambda c, d: d["M"] == 65 and "small8 MF8" in c["variant"]),
    ("W8A16 small up to 256 rows", _W8OPS, lambda c, d: d["M"] == 256 and "small8" in c["variant"], lambda c, d: d["M"] == 257 and "decode128" in c["variant"]),
    ("W8A16 MFMA from 5 rows", _W8OPS, lambda c, d: d["M"] == 4 and d["K"] == 80 and c["variant"] == "linear8_generic", lambda c, d: d["M"] == 5 and d["K"] == 80 and c["variant"] == "decode128"),
    ("W8A16 generic: 65535 rows in grid.y", _W8OPS, _m(65535, dt="f32"), _m(65536, dt="f32")),
    ("W8A16 generic, 16 bit: 65535 rows in grid.y", _W8OPS, lambda c, d: d["M"] == 65535 and d["K"] == 72, lambda c, d: d["M"] == 65536 and d["K"] == 72),
    ("k_outlier_add: 65535 row groups in grid.y", ("outlier_linear",), _m(1048560), _m(1048576)),
    ("k_gemm_mid up to 384 rows from N = 8192", _M4OPS, lambda c, d: d["M"] == 384 and d["N"] == 8192 and c["variant"] == "mid",
     lambda c, d: d["M"] == 385 and d["N"] == 8192 and c["variant"] == "decode128"),
    ("k_gemm_mid below 96 tiles of 256 x 256", _M4OPS, lambda c, d: d["tiles256"] == 94 and c["variant"] == "mid", lambda c, d: d["M"] == 300 and d["tiles256"] == 96),
    ("k_gemm_small up to K = 32768", _M4OPS, lambda c, d: d["K"] == 32768 and c["variant"].startswith("small"), lambda c, d: d["K"] == 33024 and c["kernel"] == "skinny_mfma16"),
    ("k_gemm_small from N = 64", _M4OPS, lambda c, d: d["N"] == 63 and d["K"] == 768 and c["kernel"] == "skinny_mfma16", lambda c, d: d["N"] == 64 and c["variant"].startswith("small")),
    ("the dense path from K = 128", _M4OPS, lambda c, d: d["M"] == 1024 and d["K"] == 64 and "dense" not in c["kernel"], lambda c, d: d["M"] == 1024 and d["K"] == 128 and c["kernel"] == "dequant+dense"),
    ("128 x 128 dense tiles from K = 192", _M4OPS + ("linear_int8", "matmul_fp8"), lambda c, d: d["M"] == 1024 and d["K"] == 128 and c["variant"] == "dense 256x128",
     lambda c, d: d["M"] == 1024 and d["K"] == 192 and c["variant"] == "dense 128x128"),
    ("the dense path from 10^6 outputs above 256 rows", _M4OPS, lambda c, d: d["M"] == 257 and d["N"] == 3891 and "dense" not in c["kernel"],
     lambda c, d: d["M"] == 257 and d["N"] == 3892 and c["kernel"] == "dequant+dense"),
    ("the dequantise pass in its four-row form up to 2^25 weights", _M4OPS + _W8OPS[:1], lambda c, d: d["M"] == 2048 and d["NK"] == 8065 * 4160, lambda c, d: d["M"] == 2048 and d["NK"] == 8066 * 4160),
    ("the dequantise pass write-through from 2048 rows above 2^25 weights", _M4OPS + _W8OPS, lambda c, d: d["M"] == 2047 and d["NK"] > 1 << 25, lambda c, d: d["M"] == 2048 and d["NK"] > 1 << 25),
    ("the f32 path from N = 32", _M4OPS, lambda c, d: d["dt"] == "f32" and d["N"] == 31 and c["kernel"] == "generic", lambda c, d: d["dt"] == "f32" and d["N"] == 32 and d["K"] == 16 and c["variant"] == "f32 64 x1"),
    ("the f32 path from K = 16", _M4OPS, lambda c, d: d["dt"] == "f32" and d["K"] == 12 and c["kernel"] == "generic", lambda c, d: d["dt"] == "f32" and d["K"] == 16 and c["variant"] == "f32 64 x1"),
    ("outlier_linear's row quantiser in registers up to K = 8192", ("outlier_linear",), lambda c, d: d["K"] == 8192, lambda c, d: d["K"] == 8208),
]

# every literal of INTEGER_LIMITS (below) -> the THRESHOLDS row that stands on both of its sides, or ("no case", why) where no call can
# stand on one side of it alone
_NO = "no case"
LIMIT_CLAIMS = {
    "matmul4_kernels.hip": {1: "k_gemv4 M = 1 | 2", 2: "k_gemv4 M = 1 | 2", 3: "lean GEMV ku <= 4 on its own KU, ku 5 on KU = 6", 4: "k_gemv4 M <= 4 | 5",
                            6: "lean GEMV ku <= 6 on KU = 6, ku 7 on KU = 8", 8: "lean GEMV up to K = 16384 (ku <= 8)", 16: "GEMV M <= 16 | 17",
                            24: "skinny at 33 <= M <= 64 up to N * K = 2^24", 32: "skinny MT: M <= 32 | 33", 64: "skinny up to M = 64",
                            96: "96 tiles of 256 x 256, fused", 1024: "lean GEMV from K = 1024", 8192: "k_gemv4 two rows per wave from N = 8192"},
    "int8_kernels.hip": {1: (_NO, "M >= 1 holds for every call that reaches a launcher"), 4: "W8A16 MFMA from 5 rows", 16: "skinny MT: M <= 16 | 17",
                         32: "W8A16 small from 33 rows", 64: "W8A16 small MF: M <= 64 | 65", 256: "W8A16 small up to 256 rows", 65535: "W8A16 generic: 65535 rows in grid.y"},
    "gemm_dense.hip": {8: (_NO, "cost model: at most 8 slices of at least 8 steps (gemm_dense_plan)"), 25: "the dequantise pass in its four-row form up to 2^25 weights",
                       31: (_NO, "size guard: 256 rows of K need 2 GiB, K >= 2^22"), 96: "96 tiles of 256 x 256, the dense plan", 128: "the dense path from K = 128",
                       192: "128 x 128 dense tiles from K = 192", 256: "the dense path from 256 rows and 1.5 M outputs", 2048: "the dequantise pass write-through from 2048 rows above 2^25 weights",
                       1000000: "the dense path from 10^6 outputs above 256 rows", 1500000: "the dense path from 256 rows and 1.5 M outputs"},
    "gemm_small.hip": {8: "k_gemm_small MAXS: more than 8 steps a slice", 16: "k_gemm_small from 17 rows above 2^24 weights", 24: "k_gemm_small from 17 rows above 2^24 weights",
                       25: (_NO, "cost model: the dequantise boundary in gemm_small_one_round's estimate"), 64: "k_gemm_small from N = 64",
                       128: (_NO, "cost model: tiles2 <= 128 picks a step time in gemm_small_one_round's estimate"), 256: "k_gemm_small MF = 8 from 257 rows", 512: "k_gemm_small up to 512 rows"},
    "gemm_small8.hip": {8: (_NO, "the fallback without a workspace: functional.py always passes the one the query asks for"), 64: "W8A16 small MF: M <= 64 | 65"},
    "gemm_mid.hip": {32: (_NO, "M > 32: up to 64 rows the skinny kernel or k_gemm_small is taken first"), 96: "k_gemm_mid below 96 tiles of 256 x 256",
                     256: (_NO, "K >= 256: the launcher asks for K_weight % 256 == 0 first"), 8192: "k_gemm_mid up to 384 rows from N = 8192"},
    "gemm_fused4.hip": {128: (_NO, "K >= 128: K_weight % 256 == 0 at blocksize 64 implies it")},
    "gemm_f32.hip": {5: (_NO, "M >= 5: the cost inequality of gemm_f32_shape needs more than 8 rows at every N and K"), 16: "the f32 path from K = 16", 32: "the f32 path from N = 32"},
    "nn_kernels.hip": {8192: "outlier_linear's row quantiser in registers up to K = 8192"},
}

# (op, the variant an aligned call takes) -> the variant the same call takes with its activation 2 bytes off 16-byte alignment
# (view = "misaligned"); OPERAND_ALIGNMENT_TESTED does the same for the other operands.  Only the workspaces, which functional.py
# allocates itself, and absmax2 cannot be offset through the public ops.
ALIGNMENT_TESTED = {
    ("matmul_4bit", "gemv_lean ku2/KU2"): "generic ROWS1 flags1",          # fast_layout: aligned16(A)
    ("matmul_4bit", "skinny MT1 NR1"): "generic ROWS8 flags1",
    ("matmul_4bit", "dense 256x128"): "generic ROWS8 flags1",               # matmul_4bit_dense_path's own test first
    ("linear_int8", "skinny8 MT1"): "linear8_generic",
    ("linear_int8", "small8 MF4 x1"): "linear8_generic",                    # launch_gemm_small8's own test first
    ("linear_int8", "dense 256x128"): "linear8_generic",                    # linear8_dense_path's
    ("matmul_fp8", "skinny8 MT1"): "linear8_generic",
    ("matmul_fp8", "small8 MF4 x1"): "linear8_generic",
    ("matmul_fp8", "dense 256x128"): "linear8_generic",
}
# (op, view, the aligned call's variant) -> the variant with that one operand off its alignment
OPERAND_ALIGNMENT_TESTED = {
    ("matmul_4bit", "absmax+4", "fused4"): "gemm256p am4",                   # matmul_4bit_fused4_path: a 16-byte aligned f32 absmax
    ("matmul_4bit", "packed+4", "skinny MT1 NR1"): "generic ROWS8 flags3",   # fast_layout: aligned16(packed)
    ("matmul_4bit", "packed+2", "generic ROWS4 flags3"): "generic ROWS4 flags2",   # the generic kernel's dword loads of `packed`
    ("matmul_4bit", "packed+2", "dense 256x128"): "generic ROWS8 flags2",    # matmul_4bit_dense_path: packed & 3
    ("matmul_4bit", "codes+1", "gemv_lean ku6/KU6"): "gemv MT1 NR1 KU2 regs",    # am.i8 & 3, the lean GEMV
    ("matmul_4bit", "codes+1", "mid"): "decode128",                          # ... k_gemm_mid
    ("matmul_4bit", "codes+1", "fused4"): "gemm256p",                        # ... fused4 and AM4
    ("matmul_4bit", "misaligned", "f32 64 x1"): "generic ROWS8 flags1",      # matmul_4bit_f32_path's A, the generic kernel's xvec
    ("linear_int8", "w+1", "skinny8 MT1"): "linear8_generic", ("matmul_fp8", "w+1", "skinny8 MT1"): "linear8_generic",
    ("linear_int8", "w+1", "small8 MF4 x1"): "linear8_generic", ("matmul_fp8", "w+1", "small8 MF4 x1"): "linear8_generic",
    ("linear_int8", "w+1", "decode128"): "linear8_generic", ("matmul_fp8", "w+1", "decode128"): "linear8_generic",
    ("matmul_int8", "a+1", "i8_dense"): "",                                  # i8_generic
    ("matmul_int8", "b+1", "i8_dense"): "",                                  # the generic transpose + i8_mfma256
}

# change detectors (tests/test_gemm_variants_host.py): the pointer tests (aligned16 / reinterpret_cast<uintptr_t>) of every GEMM launcher
# file, and the integer literals its code compares M, N, K, K_weight, a tile, step or workgroup count, N * K or M * N with.  One that is
# added or removed breaks the count until THRESHOLDS / ALIGNMENT_TESTED and their cases follow.  nn_kernels.hip's seven pointer tests and
# its other limits each have a pair of cases in tests/nn_cases.py (ALIGNMENT_TESTED and THRESHOLDS there).
ALIGNMENT_TEST_COUNTS = {"matmul4_kernels.hip": 13, "int8_kernels.hip": 17, "gemm_dense.hip": 6, "gemm_small.hip": 1, "gemm_small8.hip": 3,
                         "gemm_mid.hip": 1, "gemm_fused4.hip": 5, "gemm_f32.hip": 2, "nn_kernels.hip": 7}
INTEGER_LIMITS = {
    "matmul4_kernels.hip": [1, 2, 3, 4, 6, 8, 16, 24, 32, 64, 96, 1024, 8192],
    "int8_kernels.hip": [1, 4, 16, 32, 64, 256, 65535],
    "gemm_dense.hip": [8, 25, 31, 96, 128, 192, 256, 2048, 1000000, 1500000],
    "gemm_small.hip": [8, 16, 24, 25, 64, 128, 256, 512],
    "gemm_small8.hip": [8, 64],
    "gemm_mid.hip": [32, 96, 256, 8192],
    "gemm_fused4.hip": [128],
    "gemm_f32.hip": [5, 16, 32],
    "nn_kernels.hip": [8192],
}
