"""CPU check that the engine's environment knobs and INTEGRATION.md's
"Runtime knobs" table list each other (the sources are read as text):

  * every "OPENR_..." literal the engine sources hand to getenv or one of the
    env_* readers has a row in the table;
  * every OPENR_NL_* / OPENR_MS_* / OPENR_SPF_* row of the table is still
    read somewhere under openr_amd/ (a retired knob loses its row).
"""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openr_amd")
ENGINE = [os.path.join(PKG, "csrc", f) for f in ("spf_device.hip", "spf_cluster.hip")]
SOURCE_SUFFIXES = (".py", ".hip", ".cpp", ".h")


def _table_knobs():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## Runtime knobs"):].split("\n## ", 1)[0]
    names = set()
    for line in section.splitlines():
        if line.startswith("|"):
            first_cell = line.split("|")[1]
            names.update(re.findall(r"\bOPENR_[A-Z0-9_]+", first_cell))
    return names


def _engine_reads():
    reads = set()
    for path in ENGINE:
        text = open(path).read()
        reads.update(re.findall(r'\b(?:getenv|env_[a-z0-9_]+)\s*\(\s*"(OPENR_[A-Z0-9_]+)"', text))
    return reads


def _package_literals():
    found = set()
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(SOURCE_SUFFIXES):
                text = open(os.path.join(d, f), errors="replace").read()
                found.update(re.findall(r'"(OPENR_[A-Z0-9_]+)"', text))
    return found


def test_every_engine_knob_is_documented():
    reads = _engine_reads()
    assert len(reads) > 20, "the knob pattern no longer matches the engine sources"
    assert reads <= _table_knobs(), sorted(reads - _table_knobs())


def test_every_documented_engine_knob_is_read():
    rows = {k for k in _table_knobs() if re.match(r"OPENR_(NL|MS|SPF)_", k)}
    assert len(rows) > 20, "the knob table was not found in INTEGRATION.md"
    assert rows <= _package_literals(), sorted(rows - _package_literals())
