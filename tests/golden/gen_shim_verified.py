"""Verifies shim/go/apply_shim.py against a checkout of the reference and writes tests/golden/shim_verified.json, the record
tests/test_go_shim_apply.py holds the edit list to.  The checks are the ones that need the reference's Go files: every edit finds its
method and the edited files stay well-formed; every free identifier of a replacement body is declared where the body lands.  The record
holds only counts and the sha256 of each edit (this repository's signature pattern and body), no reference text.
usage: python tests/golden/gen_shim_verified.py REFERENCE_CHECKOUT"""
import hashlib
import importlib.util
import json
import re
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "shim_verified.json"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def edit_digest(sig: str, body: str) -> str:
    return hashlib.sha256((sig + "\0" + body).encode()).hexdigest()


def verify(ref: Path) -> dict:
    shim = _load("apply_shim", ROOT / "shim" / "go" / "apply_shim.py")
    t = _load("test_go_shim_apply", ROOT / "tests" / "test_go_shim_apply.py")  # the identifier readers the test uses
    with tempfile.TemporaryDirectory() as tmp:
        done = shim.apply(ref, Path(tmp))
        assert sum(n for _, n in done) == 12 and len(done) == 8
        for rel, _ in done:
            new = (Path(tmp) / rel).read_text()
            assert new.count("{") == new.count("}")
            assert ".spx." in new or "ts.order[" in new
        tlp = (Path(tmp) / "pkg/trimaran/targetloadpacking/targetloadpacking.go").read_text()
        assert "pl.spx.ScoreRow(pod, spx.PluginTLP)" in tlp and "PredictUtilisation(&container)" not in tlp.split("func (pl *TargetLoadPacking) Score")[1].split("\nfunc ")[0]
    checked = 0
    for rel, edits in shim.EDITS.items():
        text = (ref / rel).read_text()
        known = t._package_names((ref / rel).parent) | t._imports(text) | {"spx", "fmt", "fwk"}
        for sig, body in edits:
            m = re.search(sig, text, re.M | re.S)
            assert m, (rel, sig)
            free = t._free_identifiers(body) - known - t._signature_names(m.group(0))
            assert not free, (rel, m.group(0)[:60], sorted(free))
            checked += 1
    assert checked == 12
    # the defect round 3 shipped is caught: `nodeName` is a local of the body that was replaced
    rel = "pkg/networkaware/networkoverhead/networkoverhead.go"
    sig = [s for s, _ in shim.EDITS[rel] if "Score" in s][0]
    text = (ref / rel).read_text()
    m = re.search(sig, text, re.M | re.S)
    known = t._package_names((ref / rel).parent) | t._imports(text) | {"spx", "fmt", "fwk"}
    assert "nodeName" in t._free_identifiers("\treturn row[no.spx.Column(nodeName)], nil") - known - t._signature_names(m.group(0))
    return {"files": len(done), "bodies_replaced": sum(n for _, n in done), "bodies_identifier_checked": checked,
            "edits": {rel: [edit_digest(s, b) for s, b in edits] for rel, edits in shim.EDITS.items()}}


if __name__ == "__main__":
    rec = verify(Path(sys.argv[1]))
    OUT.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(f"{OUT.name}: {rec['files']} files, {rec['bodies_replaced']} bodies verified")
