"""Coverage ratchet: every public wrapper in inklayer_amd/ops.py that launches native code is called, as
`ops.<name>`, by some test module.  A new kernel wrapper without a test fails the CPU suite."""
import ast
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# wrapper -> why it needs no `ops.<name>` call of its own
EXEMPT = {
    "mask_cleanup": "called through refine.clean_masks, which tests/test_refine_gpu.py checks bit-exactly against the oracle",
}


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


def test_exemptions_are_current():
    wrappers = set(_native_wrappers())
    for name, reason in EXEMPT.items():
        assert name in wrappers, f"{name} is exempt but is no longer a native wrapper in ops.py"
        assert reason.strip(), f"{name} is exempt without a reason"
