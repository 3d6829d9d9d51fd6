"""Shared test helpers live in tests/support.py: no file under tests/ imports a test module, and support.py holds no test."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def imported_modules(node):
    if isinstance(node, ast.Import):
        return [a.name for a in node.names]
    return [node.module or ""] if isinstance(node, ast.ImportFrom) else []


def test_no_test_module_is_imported_and_support_holds_no_test():
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        name = os.path.basename(path)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            from_tests = [m for m in imported_modules(node) if m.split(".")[-1].startswith("test_")]
            assert not from_tests, (name, node.lineno, from_tests)
            if name == "support.py" and isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                assert not node.name.startswith("test_"), node.name
