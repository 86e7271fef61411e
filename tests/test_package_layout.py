"""A private name stays private to its module: no module of the package imports an underscore name from another one (the shared
plumbing has public homes: device.py, scans.py, hip.py).  The sources are parsed, nothing is imported."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_module_imports_a_private_name_of_another():
    files = sorted(glob.glob(os.path.join(ROOT, "seggroup_amd", "*.py")))
    assert len(files) > 20
    found = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and (node.level >= 1 or node.module.startswith("seggroup_amd.")):
                found += ["%s:%d: from %s import %s" % (os.path.basename(path), node.lineno, "." * node.level + node.module, a.name)
                          for a in node.names if a.name.startswith("_")]
    assert not found, "\n".join(found)


def test_worker_count_is_clamped_in_one_place():
    from seggroup_amd import scans
    assert scans.MAX_WORKERS == 16
    assert [scans.worker_count(w, n) for w, n in ((3, 5), (99, 5), (99, 40), (0, 5), (4, 0), (-2, 0))] == [3, 5, 16, 1, 1, 1]
