"""Coverage ratchet: every public wrapper in inklayer_amd/ops.py that launches native code is called, as
`ops.<name>`, by some test module.  A new kernel wrapper without a test fails the CPU suite.

Native code that a module other than ops.py calls itself, as `_lib.lib().ink_<symbol>(...)` or through a name bound to
`_lib.lib()` (today: refine_stage.py), is held to the same rule per SYMBOL: a device entry point is called by that name
in an op-level GPU test module (tests/test_*_ops_gpu.py, where every launch is compared on its own), a host function
(ink_host_*) in any test module."""
import ast
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# wrapper -> why it needs no `ops.<name>` call of its own
EXEMPT = {
    "_resize_u8": "private: the one C call behind ops.resize_bilinear_u8 and ops.inp_resize_u8, which tests/test_resize.py "
                  "and tests/test_inpaint_gpu.py check against Pillow bit for bit",
}


# symbol called outside ops.py -> why it needs no call by name in a test module
EXEMPT_SYMBOLS = {
    "ink_host_sparse_sample": "refine_stage.sparse_sketch_sample is nothing but this call (with the retry on a full "
                              "buffer); tests/test_refine_stage_cpu.py checks it sample for sample against the oracle",
    "ink_host_assign_unlabeled": "refine_stage.assign_unlabeled is nothing but this call; "
                                 "tests/test_refine_stage_cpu.py checks it pixel for pixel against the oracle",
}


def _is_lib_call(node):
    return isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "lib"


def _direct_symbols(path: Path):
    """Names `ink_x` of every call `_lib.lib().ink_x(...)` or `L.ink_x(...)`, L a name assigned from `_lib.lib()`."""
    tree = ast.parse(path.read_text())
    bound = {t.id for node in ast.walk(tree) if isinstance(node, ast.Assign) and _is_lib_call(node.value)
             for t in node.targets if isinstance(t, ast.Name)}
    return {node.func.attr for node in ast.walk(tree)
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("ink_")
            and (_is_lib_call(node.func.value) or (isinstance(node.func.value, ast.Name) and node.func.value.id in bound))}


def _symbols_called_outside_ops():
    return sorted(set().union(*(_direct_symbols(p) for p in sorted((ROOT / "inklayer_amd").glob("*.py"))
                                if p.name not in ("ops.py", "_lib.py"))))


def _native_wrappers():
    tree = ast.parse((ROOT / "inklayer_amd" / "ops.py").read_text())
    names = []
    for node in tree.body:
        if not isinstance(node, ast.FunctionDef):
            continue
        for sub in ast.walk(node):      # _lib.lib().ink_<symbol>
            if (isinstance(sub, ast.Attribute) and sub.attr.startswith("ink_") and isinstance(sub.value, ast.Call)
                    and isinstance(sub.value.func, ast.Attribute) and sub.value.func.attr == "lib"):
                names.append(node.name)
                break
    return names


def _ops_calls(path: Path):
    """Names `n` of every call `ops.n(...)` in the code of a test module (comments and strings do not count)."""
    return {node.func.attr for node in ast.walk(ast.parse(path.read_text()))
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
            and isinstance(node.func.value, ast.Name) and node.func.value.id == "ops"}


def test_every_native_wrapper_has_a_test():
    wrappers = _native_wrappers()
    assert len(wrappers) >= 30 and "msda_fused" in wrappers and "gemm" in wrappers   # the parse found them
    me = Path(__file__).name
    called = set().union(*(_ops_calls(p) for p in sorted((ROOT / "tests").glob("test_*.py")) if p.name != me))
    untested = [n for n in wrappers if n not in EXEMPT and n not in called]
    assert not untested, f"native wrappers without a test calling ops.<name>(...): {untested}"


def test_every_symbol_called_outside_ops_has_a_test():
    symbols = _symbols_called_outside_ops()
    assert len(symbols) >= 12 and "ink_refine_grow" in symbols and "ink_host_sparse_sample" in symbols   # the parse found them
    me = Path(__file__).name
    tests = [p for p in sorted((ROOT / "tests").glob("test_*.py")) if p.name != me]
    anywhere = set().union(*(_direct_symbols(p) for p in tests))
    op_level = set().union(*(_direct_symbols(p) for p in tests if p.name.endswith("_ops_gpu.py")))
    untested = [n for n in symbols if n not in EXEMPT_SYMBOLS
                and n not in (anywhere if n.startswith("ink_host_") else op_level)]
    assert not untested, f"native symbols called outside ops.py without an op-level test calling them by name: {untested}"


def test_exemptions_are_current():
    wrappers = set(_native_wrappers())
    for name, reason in EXEMPT.items():
        assert name in wrappers, f"{name} is exempt but is no longer a native wrapper in ops.py"
        assert reason.strip(), f"{name} is exempt without a reason"
    symbols = set(_symbols_called_outside_ops())
    for name, reason in EXEMPT_SYMBOLS.items():
        assert name in symbols, f"{name} is exempt but no module outside ops.py calls it any more"
        assert reason.strip(), f"{name} is exempt without a reason"
