"""
The kernel routes of libmbnb_train.so (include/mbnb_train.h), one table.  Each case names an op, a shape, a dtype and the name
mbnb_train_last_kernel() must report for it.  Data only, importable without a GPU: tests/test_gpu_switchback.py runs every case and
checks every output element against float64 (tests/elementwise.py); tests/test_switchback_host.py checks that every name the library
can report (its kTrainKernelNames table) is the kernel of some case.

Keys
  op       forward (functional._switchback_forward), dequant (its Wd pass alone), grad_w (functional._linear_grad_weight),
           transpose (its transposing pass alone)
  M N K    rows (tokens), output columns, input columns; lead: the leading dims of a 3-D input instead of M
  dt       "f16" | "bf16" | "f32";  bias: with a bias;  generic: MBNB_TRAIN_FORCE_GENERIC
  view     "misaligned": the activation (and dY) 2 bytes off 16-byte alignment
"""


def _c(op, kernel, **kw):
    kw.update(op=op, kernel=kernel)
    return kw


FORWARD = [
    _c("forward", "switchback_dq+dense", M=512, N=3072, K=512, dt="bf16", bias=True),      # 16-byte bias epilogue
    _c("forward", "switchback_dq+dense", M=300, N=5003, K=192, dt="f16", bias=True),       # ragged N: scalar bias epilogue
    _c("forward", "switchback_dq+dense", M=1024, N=2048, K=1024, dt="f16"),
    _c("forward", "switchback_dq+dense", lead=(4, 128), N=4096, K=256, dt="bf16", bias=True),   # 3-D input
    _c("forward", "switchback_dq+dense", M=16, N=4096, K=4096, dt="f16", bias=True),
    _c("forward", "switchback_dq+dense", M=1, N=16384, K=8192, dt="bf16", bias=True),
    _c("forward", "switchback_generic", M=1, N=4096, K=4096, dt="bf16", bias=True),
    _c("forward", "switchback_generic", M=1, N=257, K=100, dt="f16"),
    _c("forward", "switchback_generic", M=17, N=100, K=100, dt="f16", bias=True),
    _c("forward", "switchback_generic", M=64, N=256, K=512, dt="f32", bias=True),
    _c("forward", "switchback_generic", M=600, N=3072, K=512, dt="f32"),
    _c("forward", "switchback_generic", lead=(2, 5), N=72, K=136, dt="bf16", bias=True),
    _c("forward", "switchback_generic", M=512, N=3072, K=512, dt="f16", bias=True, generic=True),
    _c("forward", "switchback_generic", M=512, N=3072, K=512, dt="bf16", view="misaligned"),
    _c("forward", "switchback_generic", M=512, N=3000, K=500, dt="bf16", bias=True),       # K % 64 != 0
]
DEQUANT = [
    _c("dequant", "switchback_dq", N=4096, K=4096, dt="f16"),
    _c("dequant", "switchback_dq", N=11008, K=4096, dt="bf16"),      # more than 2^25 elements: one row per thread
    _c("dequant", "switchback_dq", N=1000, K=1000, dt="bf16"),
    _c("dequant", "switchback_dq", N=77, K=100, dt="f16"),           # K % 8 != 0: the scalar pass
    _c("dequant", "switchback_dq", N=33, K=64, dt="f32"),
]
GRAD_W = [
    _c("grad_w", "grad_w_t+dense", M=1, N=8192, K=8256, dt="bf16"),
    _c("grad_w", "grad_w_t+dense", M=17, N=4096, K=4096, dt="f16"),
    _c("grad_w", "grad_w_t+dense", M=100, N=1024, K=2048, dt="bf16"),
    _c("grad_w", "grad_w_t+dense", M=4095, N=1024, K=2048, dt="f16"),
    _c("grad_w", "grad_w_t+dense", M=4096, N=1024, K=2048, dt="bf16"),
    _c("grad_w", "grad_w_t+dense", M=333, N=1001, K=1537, dt="f16"),                 # ragged N and K: 2-byte loads
    _c("grad_w", "grad_w_t+dense", lead=(3, 70), N=2048, K=1024, dt="bf16", view="misaligned"),
    _c("grad_w", "grad_w_generic", M=1, N=1024, K=2048, dt="bf16"),
    _c("grad_w", "grad_w_generic", M=17, N=1024, K=2048, dt="f16"),
    _c("grad_w", "grad_w_generic", M=100, N=256, K=512, dt="f32"),
    _c("grad_w", "grad_w_generic", M=7, N=40, K=100, dt="f16"),
    _c("grad_w", "grad_w_generic", M=1, N=96, K=64, dt="bf16"),
    _c("grad_w", "grad_w_generic", M=333, N=512, K=4096, dt="bf16", generic=True),
]
TRANSPOSE = [
    _c("transpose", "grad_w_t", M=4096, K=4096, dt="bf16"),
    _c("transpose", "grad_w_t", M=1, K=1024, dt="f16"),
    _c("transpose", "grad_w_t", M=100, K=1537, dt="f16"),            # ragged: 2-byte loads, 36 zero columns
    _c("transpose", "grad_w_t", M=4095, K=72, dt="bf16"),
]
CASES = FORWARD + DEQUANT + GRAD_W + TRANSPOSE


def case_id(c):
    rows = "x".join(map(str, c["lead"])) if "lead" in c else str(c.get("M", ""))
    parts = [c["op"], c["kernel"], rows, str(c.get("N", "")), str(c["K"]), c["dt"]]
    parts += [k for k in ("bias", "generic") if c.get(k)] + ([c["view"]] if "view" in c else [])
    return "-".join(p for p in parts if p)
