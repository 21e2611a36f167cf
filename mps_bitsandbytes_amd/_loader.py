"""
The one load path of the nine native libraries.  A binding module (_native, _optim_native, _train_native, _sparse_native,
_paged_native, _group_native, _lora_native, _batch_native, _mlora_native) keeps what is its own -- LIB_PATH, ABI_VERSION, _PREFIX (of its `*_abi_version` / `*_last_error` exports), _CHECK_PREFIX (of check()'s
message), _SIGNATURES, optionally _REQUIRES (binding modules whose library is loaded first), and the cache `_lib` / `_load_error` -- and a three-line `lib()`
that returns the cached handle itself, so a call on the hot path never comes here.  Everything else works on that module's globals,
read at the time of the call: assigning LIB_PATH (or clearing the cache) on the module redirects the next load.

There is NO Python/CPU fallback behind any of the libraries: a missing library or a failed call is a RuntimeError.
"""
import ctypes
import os

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


def failed(g: dict, status: int, what: str) -> RuntimeError:
    """The error of a call that returned `status` != 0, with the library's own last-error text."""
    msg = getattr(g["lib"](), g["_PREFIX"] + "_last_error")().decode(errors="replace")
    return RuntimeError(f"{g['_CHECK_PREFIX']}.{what} failed (status {status}): {msg}")
