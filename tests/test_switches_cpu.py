"""Every environment variable the product code or the bench reads (getenv / os.environ) and every compile-time
A/B switch of the HIP sources (#ifndef USV_*) is documented in INTEGRATION.md's switches tables, and every switch
those tables document still exists in the sources."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omniisaacgymenvs_loop_amd")


def _sources():
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                yield os.path.join(d, f)
    yield os.path.join(ROOT, "bench.py")


def test_every_switch_is_documented():
    env_re = re.compile(r"""(?:getenv|environ\.get)\(\s*["'](USV_[A-Z0-9_]+)["']""")
    ifndef_re = re.compile(r"^#ifndef (USV_[A-Z0-9_]+)\s*$", re.M)
    names = set()
    for p in _sources():
        text = open(p, encoding="utf-8").read()
        names.update(env_re.findall(text))
        if p.endswith(".hip"):
            names.update(n for n in ifndef_re.findall(text) if not n.endswith("_H"))
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert names, "no switches found: the scan is broken"
    missing = sorted(n for n in names if f"`{n}`" not in doc)
    assert not missing, f"switches missing from INTEGRATION.md: {missing}"


def test_every_documented_switch_exists():
    """The converse: every name in the first column of the two switches tables (not the retired list below them)
    occurs in the package sources or bench.py, by plain text search."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    section = doc.split("## Runtime and build switches", 1)[1].split("\n#", 1)[0]
    rows = [line for line in section.splitlines() if line.startswith("| `USV_")]
    names = {n for line in rows for n in re.findall(r"`(USV_[A-Z0-9_]+)`", line.split("|")[1])}
    assert len(rows) >= 30 and len(names) >= len(rows), "no switch tables found: the scan is broken"
    text = "\n".join(open(p, encoding="utf-8").read() for p in _sources())
    stale = sorted(n for n in names if not re.search(rf"\b{n}\b", text))
    assert not stale, f"INTEGRATION.md documents switches that no source reads: {stale}"
