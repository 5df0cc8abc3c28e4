"""Shared test helpers live in support modules (tests/sim_cfg.py, state_sets.py, gpu_util.py, the *_numpy.py / *_ref.py references, ...):
no file under tests/ or tools/, nor bench.py, imports a module named tests.test_*.  No exceptions."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _test_modules(node):
    """the tests.test_* modules a node imports: import / from-import statements, __import__ and import_module calls with a literal"""
    if isinstance(node, ast.ImportFrom) and node.level == 0:
        names = [node.module or ""] + ["%s.%s" % (node.module, a.name) for a in node.names]
    elif isinstance(node, ast.Import):
        names = [a.name for a in node.names]
    elif (isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", None)) in ("__import__", "import_module")
          and node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str)):
        names = [node.args[0].value]   # ("tests.conftest" is no test module: the three free_port look-ups pass)
    else:
        return []
    return sorted({".".join(n.split(".")[:2]) for n in names if n.startswith("tests.test_")})


def test_no_file_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))) + [os.path.join(ROOT, "bench.py")]
    assert len(files) > 100
    bad = ["%s:%d imports %s" % (os.path.relpath(path, ROOT), node.lineno, m)
           for path in files for node in ast.walk(ast.parse(open(path).read())) for m in _test_modules(node)]
    assert not bad, bad
