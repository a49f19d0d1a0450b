"""provekit_amd -- MI355X (gfx950) backend for ProveKit's WHIR prover hot path.

The product is libprovekit_hip.so (hand-written HIP behind the C ABI in
include/provekit_hip.h); this package is the thin host layer that mirrors the
reference's plug-in interfaces for that path.  See DESIGN.md.
"""
from ._lib import LIB_PATH, PK_COL_MAJOR, PK_LEAF_MAJOR, ProveKitHipError  # noqa: F401
from .runtime import Context, DeviceBuffer, default_context  # noqa: F401


def __getattr__(name):
    # ProofEngine lives in a library of its own (libprovekit_engine.so); it is loaded when first asked for, so a caller of the product
    # library alone never needs it -- and one who asks for it without the built library gets engine.py's ImportError
    if name == "ProofEngine":
        from .engine import ProofEngine

        return ProofEngine
    if name == "Verifier":  # likewise libprovekit_verify.so
        from .verify import Verifier

        return Verifier
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
