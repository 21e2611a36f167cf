"""
The one load path of the fourteen native libraries.  A binding module (_native, _optim_native, _train_native, _sparse_native,
_paged_native, _group_native, _lora_native, _batch_native, _mlora_native, _mx_native, _moe_native, _moemlp_native, _router_native, _moegemm_native) keeps what is its own -- LIB_PATH, ABI_VERSION, _PREFIX (of its `*_abi_version` / `*_last_error` exports), _CHECK_PREFIX (of check()'s
message), _SIGNATURES, optionally _REQUIRES (binding modules whose library is loaded first), and the cache `_lib` / `_load_error` -- and a three-line `lib()`
that returns the cached handle itself, so a call on the hot path never comes here.  Everything else works on that module's globals,
read at the time of the call: assigning LIB_PATH (or clearing the cache) on the module redirects the next load.  The grouped decode
bindings (_group_native, _lora_native, _batch_native, _mlora_native) also share call_chunks(), the loop that cuts their tables into
calls of at most MAX_MEMBERS members.

There is NO Python/CPU fallback behind any of the libraries: a missing library or a failed call is a RuntimeError.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def load(g: dict):
    """Load the library of the binding module whose globals are `g`, or raise what an earlier attempt raised."""
    if g["_load_error"] is not None:
        raise RuntimeError(g["_load_error"])
    path = g["LIB_PATH"]
    if not os.path.exists(path):
        g["_load_error"] = (f"mps_bitsandbytes_amd: native library {path} not found. Build it with "
                            f"`make -C {os.path.join(_HERE, 'csrc')}` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
                            f"There is no Python fallback.")
        raise RuntimeError(g["_load_error"])
    for dep in g.get("_REQUIRES", ()):
        dep.lib()              # e.g. libmbnb_hip.so first: the dependency a library resolves next to itself; its failure is the caller's
    try:
        handle = ctypes.CDLL(path)
        for name, (res, args) in g["_SIGNATURES"].items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        reported = getattr(handle, g["_PREFIX"] + "_abi_version")()
        if reported != g["ABI_VERSION"]:
            raise OSError(f"ABI version mismatch: library reports {reported}, binding expects {g['ABI_VERSION']}")
    except (OSError, AttributeError) as e:
        g["_load_error"] = f"mps_bitsandbytes_amd: cannot load {path}: {e}"
        raise RuntimeError(g["_load_error"]) from e
    g["_lib"] = handle
    return handle


def loads(lib) -> bool:
    """A binding module's available(): True when its lib() succeeds (the library is present and loads; no GPU needed)."""
    try:
        lib()
        return True
    except RuntimeError:
        return False


def call_chunks(g: dict, entry: str, what: str, head: tuple, tables, mid: tuple, stream, log_tail: tuple):
    """The grouped libraries' one call loop.  `tables` is a list of (rows, numpy record dtype, ctypes Structure), the member table
    first: every MAX_MEMBERS rows of them make one call `entry(*head, *tables, *mid, rows in the call, 0, stream)` of the binding
    module whose globals are `g`.  A call that answers NOT_APPLICABLE is not a failure: the library declined that chunk before
    launching anything.  Any other status goes through the module's check(`what`), and a call that launched is logged in its
    launch_log as (rows in the call, the sum of R of each further table, *log_tail).  Returns one flag per call: True = launched."""
    fn = getattr(g["lib"](), entry)
    step, declined = g["MAX_MEMBERS"], g["NOT_APPLICABLE"]
    done = []
    for c0 in range(0, len(tables[0][0]), step):
        parts = [np.array(rows[c0:c0 + step], dtype=record) for rows, record, _ in tables]
        pointers = [part.ctypes.data_as(ctypes.POINTER(struct)) for part, (_, _, struct) in zip(parts, tables)]
        status = fn(*head, *pointers, *mid, len(parts[0]), 0, stream)
        if status != declined:
            g["check"](status, what)
            g["launch_log"].append((len(parts[0]), *(int(part["R"].sum()) for part in parts[1:]), *log_tail))
        done.append(status != declined)
    return done


def failed(g: dict, status: int, what: str) -> RuntimeError:
    """The error of a call that returned `status` != 0, with the library's own last-error text."""
    msg = getattr(g["lib"](), g["_PREFIX"] + "_last_error")().decode(errors="replace")
    return RuntimeError(f"{g['_CHECK_PREFIX']}.{what} failed (status {status}): {msg}")
