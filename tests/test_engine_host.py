"""CPU: the proof engine is a second library ABOVE the product's C ABI -- include/provekit_engine.h, libprovekit_engine.so and
provekit_amd/engine.py agree symbol for symbol, the engine exports nothing under the product's prefix and leaves the product's
export list alone, its source reaches the product only through provekit_hip.h, and without a GPU it raises (no compute here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "provekit_engine.h")
PRODUCT_HEADER = os.path.join(ROOT, "include", "provekit_hip.h")
SELFTEST_HEADER = os.path.join(ROOT, "tools", "probes", "pk_selftest.h")
SOURCE = os.path.join(ROOT, "provekit_amd", "csrc", "engine.cpp")


def declared(header, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, src)))


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r" [TtWwBbDdRr] ([A-Za-z_][A-Za-z0-9_]*)$", nm, flags=re.M)))


def test_header_library_and_python_table_agree():
    from provekit_amd import engine

    api = declared(HEADER, "pke")
    assert "pke_engine_create" in api and "pke_prove_many" in api and "pke_submit" in api and "pke_wait" in api
    assert sorted(engine.SIGNATURES) == api
    assert [s for s in exported(engine.ENGINE_LIB_PATH) if s.startswith("pke_")] == api
    # every argument list of the table has the length the header declares
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, args) in engine.SIGNATURES.items():
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1).strip()
        want = 0 if params in ("", "void") else params.count(",") + 1
        assert len(args) == want, f"{name}: engine.py lists {len(args)} arguments, the header declares {want}"


def test_engine_adds_nothing_to_the_product_abi():
    from provekit_amd import _lib, engine

    # the engine library: its own prefix only (C++ runtime instantiations aside, nothing a binder could call)
    mine = [s for s in exported(engine.ENGINE_LIB_PATH) if not s.startswith("_Z")]
    assert [s for s in mine if s.startswith("pk_")] == []
    assert [s for s in mine if not s.startswith("pke_")] == [], "the engine exports C symbols outside its prefix"
    # the product library: exactly its header plus the self-tests, as before -- and nothing of the engine's
    product = exported(_lib.LIB_PATH)
    assert [s for s in product if s.startswith("pke_")] == []
    assert [s for s in product if s.startswith("pk_")] == sorted(declared(PRODUCT_HEADER, "pk") + declared(SELFTEST_HEADER, "pk"))
    assert len(declared(PRODUCT_HEADER, "pk")) == 103
    assert not set(engine.SIGNATURES) & set(_lib.SIGNATURES)


def test_engine_source_reaches_the_product_only_through_its_header():
    txt = open(SOURCE).read()
    quoted = re.findall(r'#\s*include\s*"([^"]+)"', txt)
    assert quoted == ["provekit_engine.h"], quoted  # which includes provekit_hip.h and nothing else of the project
    hdr_quoted = re.findall(r'#\s*include\s*"([^"]+)"', open(HEADER).read())
    assert hdr_quoted == ["provekit_hip.h"]
    local = {f for f in os.listdir(os.path.dirname(SOURCE)) if f.endswith((".hpp", ".h", ".hip"))}
    assert not [inc for inc in re.findall(r"#\s*include\s*[<\"]([^>\"]+)[>\"]", txt) if os.path.basename(inc) in local]
    # host code: no kernel, no launch, and of HIP only the runtime's C API header (for the free-memory query of lanes = 0)
    assert "__global__" not in txt and "<<<" not in txt and "__device__" not in txt
    assert [inc for inc in re.findall(r"#\s*include\s*<([^>]+)>", txt) if inc.startswith("hip/")] == ["hip/hip_runtime_api.h"]
    code0 = re.sub(r"//[^\n]*", "", txt)
    assert set(re.findall(r"\b(hip[A-Z]\w+)\s*\(", code0)) <= {"hipGetDevice", "hipSetDevice", "hipMemGetInfo", "hipGetLastError"}
    # every product call it makes is one the product header declares
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    calls = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", code))
    assert calls and calls <= set(declared(PRODUCT_HEADER, "pk")), sorted(calls - set(declared(PRODUCT_HEADER, "pk")))
    assert {"pk_prove", "pk_noir_prove", "pk_ctx_create", "pk_scheme_create", "pk_device_set_host_wait", "pk_scheme_arena_bytes"} <= calls


def test_the_package_loads_the_engine_library_only_when_asked():
    """`import provekit_amd` serves callers of the product library alone: libprovekit_engine.so is opened by the first use of
    provekit_amd.ProofEngine (or of provekit_amd.engine), not by the package import"""
    import sys

    code = ("import sys, provekit_amd; assert 'provekit_amd.engine' not in sys.modules; "
            "provekit_amd.ProofEngine; assert 'provekit_amd.engine' in sys.modules; "
            "import pytest\nwith pytest.raises(AttributeError): provekit_amd.no_such_name")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr


def test_python_engine_never_imports_the_oracle():
    txt = open(os.path.join(ROOT, "provekit_amd", "engine.py")).read()
    assert "oracle" not in txt and "pyref" not in txt


def test_no_gpu_fails_loudly():
    """Without a device ProofEngine(...) raises, in Python and at the C boundary; nothing falls back to the CPU."""
    import ctypes as C
    from types import SimpleNamespace

    import provekit_amd
    from provekit_amd import _lib, engine
    from provekit_amd.scheme import WhirConfig, _cfg_struct, blinding_config_for

    n = C.c_int(-1)
    rc = _lib.lib.pk_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    cfg_w, cfg_b = WhirConfig.for_size(9, 4.0), blinding_config_for(7, 4.0)
    r1cs = SimpleNamespace(handle=None, num_constraints=100, num_witnesses=161)
    with pytest.raises(provekit_amd.ProveKitHipError):
        provekit_amd.ProofEngine(r1cs, 9, 7, cfg_w, cfg_b, lanes=2)
    h, cw, cb = C.c_void_p(), _cfg_struct(cfg_w), _cfg_struct(cfg_b)
    rc = engine.lib.pke_engine_create(0, None, 100, 161, 9, 7, C.byref(cw), C.byref(cb), 2, 0, C.byref(h))
    assert rc < 0 and h.value is None and engine.lib.pke_create_error()


def test_rust_engine_bindings_match_the_header():
    """rust/provekit-prover-hip/src/engine_sys.rs is kept by hand (there is no Rust toolchain here): it must declare exactly the
    header's functions with the header's argument counts, and engine.rs must call only what it declares, with as many arguments"""
    src_dir = os.path.join(ROOT, "rust", "provekit-prover-hip", "src")
    decls = dict(re.findall(r"pub fn (pke_\w+)\((.*?)\) ->", open(os.path.join(src_dir, "engine_sys.rs")).read()))
    assert sorted(decls) == declared(HEADER, "pke")
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, params in decls.items():
        c_params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).strip()
        want = 0 if c_params in ("", "void") else c_params.count(",") + 1
        assert len([a for a in params.split(",") if a.strip()]) == want, name
    engine_rs = open(os.path.join(src_dir, "engine.rs")).read()
    calls = list(re.finditer(r"esys::(pke_\w+)\s*\(", engine_rs))
    assert {m.group(1) for m in calls} >= {"pke_engine_create", "pke_prove_many", "pke_engine_destroy"}
    for m in calls:
        depth, i, n_args, seen = 1, m.end(), 0, False
        while depth:
            ch = engine_rs[i]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                n_args += 1
            if not ch.isspace() and depth:
                seen = True
            i += 1
        want = len([a for a in decls[m.group(1)].split(",") if a.strip()])
        assert (n_args + 1 if seen else 0) == want, f"{m.group(1)}: engine.rs passes {n_args + 1 if seen else 0} arguments, engine_sys.rs declares {want}"
