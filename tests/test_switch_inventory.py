"""The environment switches the library reads are the ones DESIGN.md section 8
lists: a switch added without a row (or a row left behind) fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_by_library():
    csrc = os.path.join(ROOT, "parmmg_amd", "csrc")
    names = set()
    for f in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, f), encoding="utf-8") as fh:
            names |= set(re.findall(r'getenv\(\s*"(PMX_\w+)"\s*\)', fh.read()))
    return names


def _listed_in_design():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        text = fh.read()
    sec = text[text.index("\n## 8. "):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    rows = [r for r in sec.splitlines() if r.startswith("|")]
    assert rows and rows[0].replace(" ", "").startswith("|switch|readwhen|selects|"), "section 8 has no switch table"
    return {m.group(1) for r in rows[2:] for m in [re.match(r"\|\s*`(PMX_\w+)`\s*\|", r)] if m}


def test_switch_inventory():
    read, listed = _read_by_library(), _listed_in_design()
    assert read, "no getenv(\"PMX_...\") found: the scan is broken"
    assert read == listed, {"read but not listed": sorted(read - listed), "listed but not read": sorted(listed - read)}
