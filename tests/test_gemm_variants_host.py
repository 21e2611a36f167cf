"""
Host-side closure of tests/gemm_variant_cases.py over the GEMM-family launchers, without a GPU: every variant the sources can
report (set_kernel_variant in csrc/*.hip and *.h, the macro-generated ones expanded; the gradient path's through tests/grad_cases.py)
has a case and no case names another, the
Python restatement of the launchers' conditions gives every case its variant, and the INSTANTIATED, THRESHOLDS and
ALIGNMENT_TESTED tables hold.  The counts at the end change when a launcher gains or loses an alignment test or an integer limit.
"""
import glob
import os
import re

from tests import gemm_variant_cases as gv
from tests import grad_cases, kernel_cases
from tests.gemm_variant_cases import ALIGNMENT_TESTED, CASES, INSTANTIATED, THRESHOLDS, UNREACHABLE, case_id, derived, model, model_variant
from tests.test_elementwise_host import CSRC, _reported_names

ALL_CASES = kernel_cases.CASES + CASES
VARIANT_CASES = CASES + grad_cases.CASES             # every table that holds a variant of libmbnb_hip's record
ALL_UNREACHABLE = UNREACHABLE | grad_cases.UNREACHABLE
LAUNCHER_FILES = ("matmul4_kernels.hip", "int8_kernels.hip", "gemm_dense.hip", "gemm_small.hip", "gemm_small8.hip", "gemm_mid.hip",
                  "gemm_fused4.hip", "gemm_f32.hip", "nn_kernels.hip")


# ----------------------------------------------------------------------------------------------- the scan
def _call_args(src, start):
    """The top-level arguments of the call whose opening parenthesis ends at `start`, and the index behind its closing one."""
    args, depth, cur, i, quote = [], 1, "", start, False
    while depth:
        ch = src[i]
        if quote:
            quote = not (ch == '"' and src[i - 1] != "\\")
        elif ch == '"':
            quote = True
        elif ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
            if not depth:
                break
        elif ch == "," and depth == 1:
            args.append(cur.strip())
            cur, i = "", i + 1
            continue
        cur += ch
        i += 1
    args.append(cur.strip())
    return args, i + 1


def _alternatives(arg):
    """What a format argument can be: a literal -> itself; `cond ? A : B` of literals -> both; anything else -> a number (a regex)."""
    arg = re.sub(r"^\(int\)", "", arg.strip())
    if re.fullmatch(r'-?\d+|"[^"]*"', arg):
        return [re.escape(arg.strip('"'))]
    m = re.fullmatch(r'[^?]+\?\s*(-?\d+|"[^"]*")\s*:\s*(-?\d+|"[^"]*")', arg)
    if m:
        return [re.escape(m.group(1).strip('"')), re.escape(m.group(2).strip('"'))]
    if re.fullmatch(r'(?:[^?"]+\?\s*"[^"]*"\s*:\s*)+"[^"]*"', arg):               # a chain: c1 ? "a" : c2 ? "b" : "c"
        return [re.escape(lit) for lit in re.findall(r'"([^"]*)"', arg)]
    return [r"\d+"]


def _expand(fmt_args):
    """Regexes of the strings set_kernel_variant(fmt, args...) can produce."""
    fmt, args = fmt_args[0], fmt_args[1:]
    m = re.fullmatch(r'[^?"]+\?\s*("[^"]*")\s*:\s*("[^"]*")', fmt)                 # cond ? "a" : "b" as the whole format
    fmts = [m.group(1), m.group(2)] if m else [fmt]
    out = []
    for f in fmts:
        assert re.fullmatch(r'"[^"]*"', f), f"set_kernel_variant: the format {f!r} is no string literal"
        parts = re.split(r"%[ds]", f.strip('"'))
        assert len(parts) == len(args) + 1, (f, args)
        pats = [re.escape(parts[0])]
        for a, lit in zip(args, parts[1:]):
            pats = [p + alt + re.escape(lit) for p in pats for alt in _alternatives(a)]
        out += pats
    return out


def reported_variants(csrc=CSRC):
    """Every regex of a variant the sources can report.  A call inside `#define MBNB_X(P, ...)` counts once per use of MBNB_X in its
    file, its parameters replaced by the use's arguments (MBNB_LEAN, MBNB_GEMV, MBNB_SKINNY, MBNB_SKINNY8, MBNB_SMALL, MBNB_NB, ...)."""
    pats = set()
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        with open(path) as f:
            src = f.read()
        macros = {}                                      # name -> (params, body)
        for m in re.finditer(r"^#define (MBNB_\w+)\(([^)]*)\)((?:.*\\\n)*.*)\n", src, re.M):
            macros[m.group(1)] = ([p.strip() for p in m.group(2).split(",")], m.group(3), m.start(), m.end())
        for m in re.finditer(r"\bset_kernel_variant\(", src):
            args, _ = _call_args(src, m.end())
            if "const char" in args[0]:
                continue                                 # the declaration / definition
            owner = [(n, v) for n, v in macros.items() if v[2] <= m.start() < v[3]]
            if not owner:
                pats.update(_expand(args))
                continue
            name, (params, _, d0, d1) = owner[0]
            uses = [u for u in re.finditer(r"\b" + name + r"\(", src) if not d0 <= u.start() < d1]
            assert uses, f"{os.path.basename(path)}: {name} sets a variant and is never used"
            for u in uses:
                actual, _ = _call_args(src, u.end())
                assert len(actual) == len(params), (name, actual)
                sub = dict(zip(params, actual))
                pats.update(_expand([args[0]] + [sub.get(a, a) for a in args[1:]]))
    return pats


def test_the_variant_scan_sees_the_library():
    pats = reported_variants()
    assert {r"gemv_lean\ ku\d+/KU6", r"gemv\ MT4\ NR2\ KU1\ regs", r"small\ MF8\ NF2\ S16\ x\d+", r"dense_nb\ 7/6", r"dense\ 128x128",
            r"i8_dense\ OUTL2\ NCH2", r"generic\ ROWS8\ flags\d+", r"gemm256p\ am4", "gemm256", "fused4", r"skinny8\ MT4"} <= pats, sorted(pats)
    assert len([p for p in pats if p.startswith("gemv_lean")]) == 6 and len([p for p in pats if p.startswith(r"gemv\ MT")]) == 14
    assert len([p for p in pats if p.startswith(r"small\ MF")]) == 5 and len([p for p in pats if p.startswith("dense_nb")]) == 3
    # the gradient path: format x T x nested | plain x vec | scalar of the pass, format x T x O x nested | plain of the generic kernel
    assert len([p for p in pats if p.startswith(r"grad_t\ ")]) == 5 * 2 * 2 * 2 and len([p for p in pats if p.startswith(r"grad_generic\ ")]) == 5 * 3 * 3 * 2
    assert re.escape("grad_t fp8 bf16 plain scalar") in pats and re.escape("grad_generic dense f32>f16 plain") in pats


# ----------------------------------------------------------------------------------------------- closure over the variants
def test_every_variant_the_sources_report_has_a_case_and_no_case_names_another():
    pats = reported_variants()
    have = {c["variant"] for c in VARIANT_CASES}
    uncovered = sorted(p for p in pats if not any(re.fullmatch(p, v) for v in have) and p not in {re.escape(u) for u in ALL_UNREACHABLE})
    assert uncovered == [], "a launcher reports a variant that no case of tests/gemm_variant_cases.py or tests/grad_cases.py takes"
    strangers = sorted(v for v in have if v and not any(re.fullmatch(p, v) for p in pats))
    assert strangers == [], "a case names a variant the launchers never report"
    for u in ALL_UNREACHABLE:
        assert re.escape(u) in pats and u not in have, u
    # the GEMM tables alone are closed over everything but the gradient path's variants, as before
    gemm = {c["variant"] for c in CASES}
    assert all(p.startswith(("grad_t\\ ", "grad_generic\\ ")) for p in pats if not any(re.fullmatch(p, v) for v in gemm) and p not in {re.escape(u) for u in UNREACHABLE})
    assert not any(v.startswith(("grad_t ", "grad_generic ")) for v in gemm)


def test_every_case_takes_the_name_and_the_variant_the_launchers_conditions_give():
    for c in CASES:
        name, variant = model(c)
        want = c["kernel"]
        assert (name.startswith(want) if want.endswith(" ") else name == want) and variant == c["variant"], \
            f"{case_id(c)}: the launchers' conditions give {name!r} / {variant!r}"
        assert model_variant(c) == c["variant"]


def test_the_model_names_the_kernel_of_every_earlier_case_it_covers():
    """The restated conditions against the kernel-name table, which the GPU has held for longer."""
    n = 0
    for c in kernel_cases.CASES:
        if c["op"] in ("matmul_4bit", "linear_int8", "matmul_fp8", "linear_dense", "gemm_dense", "outlier_linear"):
            name = model(c)[0]
            want = c["kernel"]
            assert name.startswith(want) if want.endswith(" ") else name == want, (case_id(c), name)
            n += 1
    assert n >= 70


def test_every_name_has_a_case_for_every_value_of_every_axis_it_is_instantiated_for():
    for name, axes in INSTANTIATED.items():
        cs = [(c, derived(c)) for c in ALL_CASES if c["kernel"] == name]
        assert cs, name
        for axis, values in axes.items():
            have = {gv.axis_value(c, d, axis) for c, d in cs}
            assert set(values) <= have, f"{name}: no case with {axis} = {sorted(set(values) - have)}"
    reported = {c["kernel"] for c in CASES}
    assert reported <= set(INSTANTIATED), sorted(reported - set(INSTANTIATED))


def test_every_threshold_has_a_case_on_each_side():
    for what, ops, below, above in THRESHOLDS:
        for op in ops:
            cs = [(c, derived(c)) for c in CASES if c["op"] == op]
            assert any(below(c, d) for c, d in cs), f"{what}: no {op} case on the first side"
            assert any(above(c, d) for c, d in cs), f"{what}: no {op} case on the second side"


def test_every_alignment_tested_path_has_a_case_that_the_test_alone_sends_to_its_fallback():
    for (op, variant), fallback in ALIGNMENT_TESTED.items():
        hits = [c for c in CASES if c["op"] == op and c.get("view") == "misaligned" and c["variant"] == fallback and
                model_variant({k: v for k, v in c.items() if k != "view"}) == variant]
        assert hits, f"no misaligned {op} case takes {fallback!r} where the aligned call would take {variant!r}"
    for (op, view, variant), fallback in gv.OPERAND_ALIGNMENT_TESTED.items():
        hits = [c for c in CASES if c["op"] == op and c.get("view") == view and c["variant"] == fallback and
                model_variant({k: v for k, v in c.items() if k != "view"}) == variant]
        assert hits, f"no {op} case with {view} takes {fallback!r} where the aligned call would take {variant!r}"


def test_the_launchers_alignment_tests_and_integer_limits_are_the_ones_the_tables_know():
    """A limit or an alignment test added to a GEMM launcher breaks these counts until THRESHOLDS / ALIGNMENT_TESTED and their cases follow."""
    aligns, limits = {}, {}
    for name in LAUNCHER_FILES:
        with open(os.path.join(CSRC, name)) as f:
            src = re.sub(r"//[^\n]*", "", f.read())
        aligns[name] = len(re.findall(r"\baligned16\(|reinterpret_cast<uintptr_t>", src))
        limits[name] = sorted(set(int(v) for v in re.findall(
            r"\b(?:M|N|K|K_weight|tiles|tiles8|tiles2|tiles4|tiles256|steps|per|ku|wgs|N \* K|N \* K_weight|M \* N)\s*(?:<=|>=|<|>|==)\s*(?:\(\(int64_t\)1 << |\(int64_t\(1\) << )?(\d+)", src)))
    assert aligns == gv.ALIGNMENT_TEST_COUNTS, aligns
    assert limits == gv.INTEGER_LIMITS, limits
    rows = {t[0] for t in THRESHOLDS}
    for name, lits in gv.INTEGER_LIMITS.items():
        claims = gv.LIMIT_CLAIMS[name]
        assert sorted(claims) == lits, f"{name}: every literal is claimed by a THRESHOLDS row or listed as having no case"
        for lit, claim in claims.items():
            assert claim in rows or (isinstance(claim, tuple) and claim[0] == "no case" and claim[1]), (name, lit, claim)


def test_the_closure_fails_on_a_launcher_branch_without_a_case(tmp_path):
    """`else if (ku == 5) MBNB_LEAN(5);` in a scratch copy of the launcher: a seventh lean variant, and no case for it."""
    with open(os.path.join(CSRC, "matmul4_kernels.hip")) as f:
        src = f.read()
    assert src.count("else if (ku <= 6) MBNB_LEAN(6);") == 1
    (tmp_path / "matmul4_kernels.hip").write_text(src.replace("else if (ku <= 6) MBNB_LEAN(6);", "else if (ku == 5) MBNB_LEAN(5);\n else if (ku <= 6) MBNB_LEAN(6);"))
    pats = reported_variants(str(tmp_path))
    have = {c["variant"] for c in CASES}
    assert [p for p in pats if not any(re.fullmatch(p, v) for v in have) and "KU5" in p] == [r"gemv_lean\ ku\d+/KU5"]


def test_names_are_untouched_by_the_variants():
    """No variant is a kernel name's business: set_kernel_name is given what it was given before (the closure of test_elementwise_host.py)."""
    names, prefixes = _reported_names()
    assert prefixes == {"dense_nb "} and not any(n.startswith(("gemv_lean", "small MF", "generic ROWS")) for n in names)


def test_cases_are_well_formed():
    keys = {"op", "kernel", "variant", "M", "N", "K", "lead", "dt", "out", "qt", "bs", "bs2", "cs", "bias", "fused", "view", "xexp", "bad",
            "tile", "slices", "ldw", "n_out"}
    views = {None, "rows", "misaligned", "absmax+4", "codes+1", "packed+4", "packed+2", "w+1", "a+1", "b+1"}
    ids = [case_id(c) for c in ALL_CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for c in CASES:
        assert set(c) <= keys and "variant" in c, (case_id(c), set(c) - keys)
        assert c.get("dt", "f16") in ("f16", "bf16", "f32") and c.get("out", "f16") in ("f16", "bf16", "f32")
        lo, hi = c.get("xexp", (0, 0))
        if c.get("dt") == "bf16" and (lo, hi) != (0, 0):
            assert c.get("out", "bf16") in ("bf16", "f32") and -40 <= lo and hi <= 40
        if c.get("dt") == "f16" and (lo, hi) != (0, 0):
            assert -8 <= lo and hi <= 4
        if "bs2" in c:
            assert c.get("cs")
        assert c.get("view") in views, case_id(c)
