"""The ALS rank limit as the public surface states it (no GPU needed)."""
import os
import re

from mfhip import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_limit_is_256():
    assert L.ALS_MAX_RANK == 256


def test_header_names_256():
    """The ALS comment of include/mfhip.h (the one above mf_als_fit) names the limit."""
    with open(os.path.join(ROOT, "include", "mfhip.h")) as f:
        text = f.read()
    end = text.index("int mf_als_fit(")
    comment = text[text.rindex("/*", 0, end):end]
    assert "ALS.train(" in comment
    assert re.search(r"a rank above 256\b", comment), comment
    assert "above 128" not in comment

