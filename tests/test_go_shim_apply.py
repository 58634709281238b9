"""shim/go/apply_shim.py finds every method it replaces in the surveyed reference checkout, and the edited files stay well-formed
(braces balance, the new body is in, the old per-(pod,node) computation is out).  The shim itself cannot be compiled here (no Go
toolchain): tests/golden/gen_shim_verified.py checks the edit list against a reference checkout and records it, and these tests hold
the current list to that record."""
import importlib.util
import json
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
VERIFIED = ROOT / "tests" / "golden" / "shim_verified.json"


def _load_shim():
    spec = importlib.util.spec_from_file_location("apply_shim", ROOT / "shim" / "go" / "apply_shim.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _verified(mod):
    """the record tests/golden/gen_shim_verified.py wrote after its checks against the reference's Go files passed; every edit of the
    current list (signature pattern and body) must be one it verified"""
    spec = importlib.util.spec_from_file_location("gen_shim_verified", VERIFIED.parent / "gen_shim_verified.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rec = json.loads(VERIFIED.read_text())
    assert set(rec["edits"]) == set(mod.EDITS)
    for rel, edits in mod.EDITS.items():
        assert [gen.edit_digest(s, b) for s, b in edits] == rec["edits"][rel], f"{rel}: edits not verified against the reference (gen_shim_verified.py)"
    return rec


def test_every_edit_applies():
    mod = _load_shim()
    rec = _verified(mod)
    assert rec["bodies_replaced"] == 12 and rec["files"] == 8
    assert sum(len(e) for e in mod.EDITS.values()) == 12 and len(mod.EDITS) == 8
    for rel, edits in mod.EDITS.items():
        for _, body in edits:
            assert body.count("{") == body.count("}"), rel
        assert any(".spx." in body or "ts.order[" in body for _, body in edits), rel
    tlp = [b for s, b in mod.EDITS["pkg/trimaran/targetloadpacking/targetloadpacking.go"] if "Score" in s][0]
    assert "pl.spx.ScoreRow(pod, spx.PluginTLP)" in tlp and "PredictUtilisation(&container)" not in tlp


def test_shim_sources_name_only_exported_entry_points():
    """every C.spx_* the Go files call is declared in include/spx.h"""
    import re
    hdr = (ROOT / "include" / "spx.h").read_text()
    for f in (ROOT / "shim" / "go" / "pkg" / "spx").glob("*.go"):
        for name in set(re.findall(r"C\.(spx_[a-z_0-9]+)\(", f.read_text())):
            assert re.search(rf"\b{name}\(", hdr), (f.name, name)
        for const in set(re.findall(r"C\.(SPX_[A-Z_0-9]+)", f.read_text())):
            assert re.search(rf"#define {const}\b", hdr), (f.name, const)


# ---- what a compiler would have caught (round 3: an undefined identifier in a replacement body): every identifier a body uses
# freely — not as a selector's field, not declared in the body — must be a parameter or the receiver of the matched signature, a
# package-level name of the package the file belongs to, an imported package, or a Go predeclared name.
GO_KEYWORDS = set("break case chan const continue default defer else fallthrough for func go goto if import interface map package range return "
                  "select struct switch type var".split())
GO_PREDECLARED = set("bool byte complex64 complex128 error float32 float64 int int8 int16 int32 int64 rune string uint uint8 uint16 uint32 uint64 uintptr any "
                     "true false iota nil append cap clear close complex copy delete imag len make max min new panic print println real recover".split())


def _go_tokens(src):
    import sys
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import goparse
    return goparse.tokenize(src)


def _strip(src):
    import re
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r'"(?:\\.|[^"\\])*"', '""', src)
    return re.sub(r"`[^`]*`", '""', src)


def _free_identifiers(body):
    """identifiers used in `body` that are neither selectors' right-hand sides, struct-literal keys, nor declared inside it"""
    import re
    b = _strip(body)
    declared = set()
    for m in re.finditer(r"([A-Za-z_][\w, ]*?)\s*:=", b):          # a, b := ...  (also `for i, x := range`)
        declared.update(x.strip().split()[-1] for x in m.group(1).split(",") if x.strip())  # (`for i, x := range`: the last word of each part)
    for m in re.finditer(r"\bvar\s+((?:[A-Za-z_]\w*\s*,\s*)*[A-Za-z_]\w*)", b):   # var a, b T
        declared.update(x.strip() for x in m.group(1).split(","))
    for m in re.finditer(r"\bfunc\s*\(([^)]*)\)", b):              # parameters of function literals
        for part in m.group(1).split(","):
            names = part.strip().split()
            if names:
                declared.add(names[0].lstrip("*"))
    used = set()
    for m in re.finditer(r"(?<![\w.])([A-Za-z_]\w*)", b):
        name = m.group(1)
        after = b[m.end():m.end() + 2].lstrip()
        if after.startswith(":") and not after.startswith(":="):    # struct literal key / label
            continue
        used.add(name)
    return {u for u in used if u not in declared and u not in GO_KEYWORDS and u not in GO_PREDECLARED}


def _package_names(pkg_dir):
    import re
    names = set()
    for f in pkg_dir.glob("*.go"):
        if f.name.endswith("_test.go"):
            continue
        t = _strip(f.read_text())
        names.update(re.findall(r"^func\s+([A-Za-z_]\w*)", t, re.M))
        names.update(re.findall(r"^type\s+([A-Za-z_]\w*)", t, re.M))
        names.update(re.findall(r"^(?:var|const)\s+([A-Za-z_]\w*)", t, re.M))
        for blk in re.findall(r"^(?:var|const)\s*\((.*?)^\)", t, re.M | re.S):
            names.update(re.findall(r"^\s*([A-Za-z_]\w*)", blk, re.M))
        for blk in re.findall(r"^type\s*\((.*?)^\)", t, re.M | re.S):
            names.update(re.findall(r"^\s*([A-Za-z_]\w*)", blk, re.M))
    return names


def _imports(text):
    import re
    out = set()
    for blk in re.findall(r"^import\s*\((.*?)^\)", text, re.M | re.S) + re.findall(r'^import\s+([^\n(]+)$', text, re.M):
        for line in blk.splitlines():
            m = re.match(r'\s*(?:([A-Za-z_]\w*)\s+)?"([^"]+)"', line)
            if m:
                out.add(m.group(1) or m.group(2).rsplit("/", 1)[-1])
    return out


def _signature_names(sig_text):
    """receiver and parameter names of `func (r *T) M(a, b T1, c T2) ...`"""
    import re
    names = set()
    for group in re.findall(r"\(([^()]*)\)", sig_text)[:2]:
        for part in group.split(","):
            toks = part.strip().split()
            if toks:
                names.add(toks[0].lstrip("*"))
    return names


def test_replacement_bodies_use_only_declared_identifiers():
    """every free identifier of every replacement body is a parameter or the receiver of the matched signature, a package-level name of
    the file's package, an import or a predeclared name — checked against the reference's Go files by gen_shim_verified.py, together with
    the defect round 3 shipped (`nodeName`, a local of the replaced NetworkOverhead.Score body) being caught; here the current bodies
    must be the verified ones"""
    mod = _load_shim()
    rec = _verified(mod)
    assert rec["bodies_identifier_checked"] == 12
    assert "nodeName" in _free_identifiers("\treturn row[no.spx.Column(nodeName)], nil")


def test_shim_package_uses_only_declared_identifiers():
    """the cgo package itself: every free identifier of a function body is a parameter, a package-level name, an import or `C`"""
    import re
    pkg = ROOT / "shim" / "go" / "pkg" / "spx"
    known = _package_names(pkg) | {"C"}
    for f in pkg.glob("*.go"):
        known |= _imports(f.read_text())
    for f in pkg.glob("*.go"):
        t = _strip(f.read_text())
        for m in re.finditer(r"^func\s*(\([^)]*\))?\s*[A-Za-z_]\w*(?:\[[^\]]*\])?\s*\([^)]*\)[^{\n]*\{", t, re.M):
            start = m.end() - 1
            depth, i = 0, start
            while True:
                depth += t[i] == "{"
                depth -= t[i] == "}"
                if depth == 0:
                    break
                i += 1
            generic = set(re.findall(r"\[([A-Za-z_]\w*)\s", m.group(0)))  # type parameters: func cArray[T any]
            free = _free_identifiers(t[start:i + 1]) - known - _signature_names(m.group(0)) - generic
            assert not free, (f.name, m.group(0)[:70], sorted(free))


def test_shim_c_constants_are_untyped_integer_macros():
    """The shim assigns C.SPX_PLUGIN_* to C.int parameters and switches a Go byte on C.SPX_NRT_ST_* / C.SPX_QUOTA_ST_*: that only type-checks
    while cgo sees them as UNTYPED integer constants, i.e. object-like `#define NAME <integer literal>` in include/spx.h (an enum member or a
    `static const` would be a typed C value and need conversions).  No Go toolchain here: this is the part of the type check that can be
    made on the header (round-5 review, weak item 11)."""
    import re
    header = (ROOT / "include" / "spx.h").read_text()
    macros = dict(re.findall(r"^#define[ \t]+(SPX_[A-Z0-9_]+)[ \t]+(.+?)[ \t]*(?:/\*.*)?$", header, re.M))
    used = set()
    for f in (ROOT / "shim" / "go" / "pkg" / "spx").glob("*.go"):
        used |= set(re.findall(r"\bC\.(SPX_[A-Z0-9_]+)\b", f.read_text()))
    assert used, "the shim names no C constants?"
    for name in sorted(used):
        assert name in macros, f"{name}: not an object-like macro of spx.h (cgo would see a typed value, or nothing)"
        assert re.fullmatch(r"-?(0x[0-9a-fA-F]+|\d+)[uU]?", macros[name].strip()), (name, macros[name])
    # and as status bytes / plugin ids they must fit what the shim stores them in
    for name in used:
        v = int(macros[name].strip().rstrip("uU"), 0)
        assert 0 <= v <= 255, (name, v)


def test_integration_md_quotes_the_shim():
    """INTEGRATION.md section 3 shows the shim by quoting it: every ```go block tagged `<!-- verbatim: FILE -->` must be a contiguous
    piece of FILE (round 4's hand-written excerpt had drifted from shim/go/pkg/spx/spx.go — cgo include path, Engine fields: two
    descriptions of one uncompiled file)"""
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    md = (root / "INTEGRATION.md").read_text()
    blocks = re.findall(r"<!-- verbatim: (\S+) -->\n```go\n(.*?)```", md, re.S)
    assert len(blocks) >= 6
    for path, body in blocks:
        src = (root / path).read_text()
        assert body.rstrip("\n") in src, f"INTEGRATION.md quotes {path} but the block starting {body[:60]!r} is not in it"
    assert {p for p, _ in blocks} == {"shim/go/pkg/spx/spx.go", "shim/go/apply_shim.py"}
