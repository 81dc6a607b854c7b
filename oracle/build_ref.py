"""Recipe for oracle/_ref/ (a build product, not in git): the reference's model modules (`models.py`, `model2.py`) compiled to
bytecode, importable from oracle/_ref/ without their sources.  tests/golden/make_goldens*.py import the reference from there, and
tests/test_oracle_golden.py regenerates the committed fixtures with them.

The reference checkout is the one BASELINE.json records (`reference_path`), or $SAT_REFERENCE_DIR.  Where it is absent this makes
nothing and removes nothing."""
import json
import os
import py_compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MODULES = ("models", "model2")


def reference_checkout():
    path = os.environ.get("SAT_REFERENCE_DIR")
    if not path:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            path = json.load(f).get("reference_path")
    return path


def build():
    """compile the reference's modules into oracle/_ref/; returns the modules made (empty when the reference is absent)"""
    src = reference_checkout()
    if not src or not all(os.access(os.path.join(src, m + ".py"), os.R_OK) for m in MODULES):
        return []
    os.makedirs(REF_DIR, exist_ok=True)
    for m in MODULES:
        py_compile.compile(os.path.join(src, m + ".py"), cfile=os.path.join(REF_DIR, m + ".pyc"), doraise=True)
    return list(MODULES)


if __name__ == "__main__":
    print("oracle/_ref:", build() or "reference absent, nothing made")
