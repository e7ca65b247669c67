#!/usr/bin/env python3
"""Names the reference's src/Jets.jl defines or calls (tests/golden/reference_jets_names.json).

    python tests/golden/make_reference_names.py PATH/TO/Jets.jl/src/Jets.jl     # rewrites reference_jets_names.json next to this script

tests/test_julia_binding_static.py checks that every name julia/JetsHIP.jl imports from Jets exists in the reference.  The
reference's source is not part of this repository, so the test reads this list instead.  A name is listed when the reference
has it at the start of a line (optionally after `function`, `struct`, `mutable struct`, `abstract type` or `macro`) or
followed by `(` -- the same two rules the test applied to the source itself.
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_jets_names.json")
TOKEN = re.compile(r"[A-Za-z_\u00a0-\uffff][A-Za-z_0-9!\u00a0-\uffff]*")


def defined_or_called(src: str) -> list:
    names = set()
    for name in set(TOKEN.findall(src)):
        if re.search(r"(?m)^(?:abstract type |struct |mutable struct |function |macro )?" + re.escape(name) + r"\b", src) or \
                re.search(r"\b" + re.escape(name) + r"\(", src):
            names.add(name)
    return sorted(names)


def main(path: str) -> None:
    names = defined_or_called(open(path, encoding="utf-8").read())
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"source": "src/Jets.jl of the reference (Jets.jl)", "names": names}, f, indent=0, ensure_ascii=False)
        f.write("\n")
    print(f"{len(names)} names -> {OUT}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
