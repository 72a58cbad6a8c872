"""The layers of vae-los-angeles_amd: csrc -> mmvae.ops -> mmvae.* / src.* -> hostlib -> the command-line tools, imports running only
upward.  Every import statement is read from the syntax tree, those inside functions included; nothing is imported."""
import ast
import glob
import os

ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vae-los-angeles_amd")
SCRIPTS = ("evaluate", "reconstruct", "cluster_unmatched", "cross_validate", "trainer", "train", "train_dna2rna", "train_rna2dna")
TRAINERS = ("train", "train_dna2rna", "train_rna2dna")


def absolute_imports(path):
    """the top-level names of the modules a file imports absolutely (`from . import reconstruct` is the package's own module)"""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            found.update(alias.name.split(".")[0] for alias in node.names)
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            found.add(node.module.split(".")[0])
    return found


def library_files():
    return sorted(glob.glob(os.path.join(ROOT, "mmvae", "*.py")) + glob.glob(os.path.join(ROOT, "src", "**", "*.py"), recursive=True))


def test_the_files_are_where_the_test_looks():
    names = {os.path.relpath(p, ROOT) for p in library_files()}
    assert {"mmvae/unmatched.py", "mmvae/crossval.py", "mmvae/downstream.py", "mmvae/data.py", "src/models/__init__.py", "src/utils/losses.py"} <= names
    for s in SCRIPTS + ("hostlib",):
        assert os.path.exists(os.path.join(ROOT, s + ".py")), s


def test_the_library_imports_no_script():
    hits = {os.path.relpath(p, ROOT): sorted(absolute_imports(p) & set(SCRIPTS + ("hostlib",))) for p in library_files()}
    assert {p: h for p, h in hits.items() if h} == {}


def test_no_script_imports_another_script():
    hits = {}
    for s in SCRIPTS + ("hostlib",):
        allowed = {"trainer"} if s in TRAINERS else set()          # train*.py are the three entry points of trainer.run
        bad = sorted((absolute_imports(os.path.join(ROOT, s + ".py")) & set(SCRIPTS)) - allowed - {s})
        if bad:
            hits[s] = bad
    assert hits == {}
