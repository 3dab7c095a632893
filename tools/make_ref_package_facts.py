"""tests/golden/ref_package_facts.json from the reference package: the line lengths and SHA-256 digests of its R/ui.R, the routines its
src/RcppExports.cpp registers and which of them R/utils.R calls -- what tests/test_abi_cpu.py::test_the_one_line_edit_applies_to_the_reference_package
checks r/ui_R_269.sed against, without the package's text.  Run where the package is on disk (its src/ directory: HARMONY_REFERENCE_SRC, as for
oracle/_ref):   python tools/make_ref_package_facts.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref as oref  # noqa: E402
from test_abi_cpu import REF_PACKAGE_FACTS, ref_package_facts  # noqa: E402

if __name__ == "__main__":
    with open(REF_PACKAGE_FACTS, "w") as fh:
        json.dump(ref_package_facts(os.path.dirname(oref._REF_SRC)), fh, indent=0)
        fh.write("\n")
    print(REF_PACKAGE_FACTS)
