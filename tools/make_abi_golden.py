"""Records tests/golden/abi_layout_reference.txt: the layout dump of tests/test_abi_layout.py (offset and size of every field, every enumerator's value, the bytes of every
default-constructed settings struct) compiled against the reference's own headers, so that the ABI comparison runs on a machine without the reference tree.
usage: python tools/make_abi_golden.py        (needs /root/reference/Include)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_abi_layout as T  # noqa: E402

if __name__ == "__main__":
    assert T.HAVE_THEIRS, "needs " + T.THEIRS
    lines = T._run(T.THEIRS, T._layout_program(), "theirs")
    with open(T.GOLDEN, "w") as fp:
        fp.write("\n".join(lines) + "\n")
    print("%s: %d lines" % (os.path.relpath(T.GOLDEN, ROOT), len(lines)))
