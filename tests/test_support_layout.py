"""The layering of the test support: helpers live in plain support modules, so no module under tests/ (nor
tests/golden/make_golden.py) imports a test module."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_module_imports_a_test_module():
    paths = sorted(glob.glob(os.path.join(HERE, "*.py"))) + [os.path.join(HERE, "golden", "make_golden.py")]
    assert len(paths) > 40
    bad = []
    for path in paths:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += [(os.path.relpath(path, HERE), node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert bad == []
