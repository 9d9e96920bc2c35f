"""The contract of the CSR column-offset plan cannot drift (include/gko_cdna4.h, "The column-offset plan").

A product through the plan never reads col_idxs again, so an entry of the library that writes an index array and
does not say so (gkoc::csr_structure_written, csrc/common.hpp) makes the next product return GKOC_OK and the
product of the OLD matrix.  This file reads the sources, no device:

  * every C-ABI definition in ginkgo_amd/csrc/*.hip with a non-const index pointer parameter (I*, int32_t*,
    int64_t*, the L* / G* of the distributed files) either calls the hook in its body or stands in
    tests/csr_plan_not_notified.txt with a reason;
  * the entries that carry the hook are the entries the header's contract comment names, in both directions
    (compared by name stem: without the type suffixes);
  * the ledger holds no entry that is gone, hooked, or without a reason.
The device side of the same contract - that the hook of every route really drops the plan - is
tests/test_csr_offsets_routes_gpu.py.
"""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "ginkgo_amd" / "csrc"
HEADER = ROOT / "include" / "gko_cdna4.h"
LEDGER = ROOT / "tests" / "csr_plan_not_notified.txt"
HOOK = "csr_structure_written"

INDEX_POINTER = re.compile(r"^(?:I|L|G|int32_t|int64_t)\s*\*$")
# type suffixes of the entry names, as the macros paste them (##TN##_##IN) or as they are spelled out
SUFFIX = re.compile(r"(?:_(?:f64|f32|c128|c64|i32|i64|u64|f16|bf16|small))+$")


def strip_comments(text):
    """one pass, so that a comment sign inside a string or inside the other kind of comment starts nothing"""
    token = re.compile(r'"(?:\\.|[^"\\\n])*"|//[^\n]*|/\*.*?\*/', re.S)
    return token.sub(lambda m: m.group(0) if m.group(0).startswith('"') else " ", text)


def matching(text, start, opening, closing):
    """index behind the bracket that closes the one at `start`"""
    depth = 0
    for i in range(start, len(text)):
        if text[i] == opening:
            depth += 1
        elif text[i] == closing:
            depth -= 1
            if depth == 0:
                return i + 1
    raise AssertionError("unbalanced " + opening)


def stem_of(name):
    """gkoc_csr_transpose_##TN##_##IN, gkoc_fill_array_i32 -> gkoc_csr_transpose, gkoc_fill_array"""
    name = re.sub(r"_?##\s*\w+\s*(?:##)?", "_", name)
    name = re.sub(r"_+", "_", name).rstrip("_")
    # pasted macro parameters (TN, IN, ...) are upper case; the stem is what stands in front of the first
    name = re.sub(r"(?:_[A-Z][A-Z0-9]*)+$", "", name)
    while SUFFIX.search(name) and not re.search(r"_to_\w+$", name[-8:]):
        name = re.sub(r"_[a-z0-9]+$", "", name)
    return name


def definitions(path):
    """(name as written, stem, parameter list, body) of every C-ABI function DEFINITION of a source file"""
    text = strip_comments(path.read_text()).replace("\\\n", "\n")
    in_block = [(m.end(), matching(text, m.end() - 1, "{", "}")) for m in re.finditer(r'extern\s+"C"\s*\{', text)]
    out = []
    for m in re.finditer(r'(extern\s+"C"\s+)?\bint\s+(gkoc_[A-Za-z0-9_#\s]*?)\s*\(', text):
        if not m.group(1) and not any(a <= m.start() < b for a, b in in_block):
            continue
        close = matching(text, m.end() - 1, "(", ")")
        rest = text[close:].lstrip()
        if not rest.startswith("{"):
            continue        # a declaration
        body_start = text.index("{", close)
        body = text[body_start:matching(text, body_start, "{", "}")]
        params = [p.strip() for p in text[m.end():close - 1].split(",") if p.strip()]
        name = re.sub(r"\s+", "", m.group(2))
        out.append((name, stem_of(name), params, body))
    return out


def index_outputs(params):
    """names of the parameters that are non-const pointers to an index type"""
    names = []
    for p in params:
        mm = re.match(r"^(.*?)(\w+)$", p.replace("__restrict__", " ").strip())
        if mm and "const" not in mm.group(1) and INDEX_POINTER.match(mm.group(1).strip()):
            names.append(mm.group(2))
    return names


def scan():
    """stem -> {"files", "outputs", "hooked" (every definition of the stem calls the hook), "some_hooked"}"""
    found = {}
    for path in sorted(CSRC.glob("*.hip")):
        for name, stem, params, body in definitions(path):
            outs = index_outputs(params)
            hooked = HOOK in body
            if not outs and not hooked:
                continue
            e = found.setdefault(stem, {"files": set(), "outputs": set(), "hooked": True, "some_hooked": False})
            e["files"].add(path.name)
            e["outputs"].update(outs)
            e["hooked"] = e["hooked"] and hooked
            e["some_hooked"] = e["some_hooked"] or hooked
    return found


def ledger():
    """stem -> reason"""
    out = {}
    for line in LEDGER.read_text().splitlines():
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        name, _, reason = line.partition(":")
        assert name.strip() not in out, "twice in the ledger: " + name
        out[name.strip()] = reason.strip()
    return out


def header_names():
    """the contract comment's entries as a list of sets of name stems: {x,y} alternatives give an entry each,
    an [_optional] part gives one entry that may be spelled either way (gkoc_ell_to_csr, gkoc_fbcsr_convert_to_csr),
    and ' / _fill' is the shorthand of the comment's last line"""
    text = HEADER.read_text()
    start = text.index("CONTRACT (the same kind")
    comment = text[start:text.index("Any other writer", start)]
    comment = re.sub(r"\s*\n\s*\*\s*", " ", comment)
    comment = re.sub(r"(gkoc_\w+)_count / _fill", r"\1_count, \1_fill", comment)

    def braces(tok):
        m = re.search(r"\{([^}]*)\}", tok)
        if not m:
            return [tok]
        return [x for alt in m.group(1).split(",") for x in braces(tok[:m.start()] + alt + tok[m.end():])]

    def optional(tok):
        m = re.search(r"\[([^\]]*)\]", tok)
        if not m:
            return {stem_of(tok)}
        return optional(tok[:m.start()] + tok[m.end():]) | optional(tok[:m.start()] + m.group(1) + tok[m.end():])

    return [optional(t) for tok in re.findall(r"gkoc_[\w\[\]{},]*[\w\]}]", comment) for t in braces(tok)]


def test_parser_sees_the_known_shapes():
    """a definition inside a macro with pasted suffixes, a spelled-out one, one inside an extern "C" block, and
    a hook-free entry with an index output: if the parser went blind the other tests would pass vacuously"""
    found = scan()
    assert found["gkoc_csr_transpose"]["hooked"] and {"t_row_ptrs", "t_col_idxs"} <= found["gkoc_csr_transpose"]["outputs"]
    assert found["gkoc_convert_idxs_to_ptrs"]["hooked"] and found["gkoc_convert_idxs_to_ptrs"]["outputs"] == {"ptrs"}
    assert found["gkoc_memset"]["hooked"] and found["gkoc_free"]["hooked"] and found["gkoc_memcpy_d2d"]["hooked"]
    assert not found["gkoc_narrow_i64_to_i32"]["hooked"] and found["gkoc_narrow_i64_to_i32"]["outputs"] == {"out"}
    assert "gkoc_csr_spmv" not in found and "gkoc_memcpy_d2h" not in found
    assert len(found) > 60, sorted(found)
    assert stem_of("gkoc_fill_array_small") == "gkoc_fill_array"
    assert stem_of("gkoc_dist_split_count_##TN##_##LN##_##GN") == "gkoc_dist_split_count"


def test_every_index_writer_is_hooked_or_has_a_reason():
    found, led = scan(), ledger()
    missing = sorted(s for s, e in found.items() if e["outputs"] and not e["hooked"] and s not in led)
    assert not missing, ("entries with a non-const index pointer that neither call gkoc::csr_structure_written nor "
                         "stand in tests/csr_plan_not_notified.txt: %s" % missing)
    partly = sorted(s for s, e in found.items() if e["some_hooked"] and not e["hooked"])
    assert not partly, "only some definitions (value types) of these entries call the hook: %s" % partly


def test_every_hooked_output_is_hooked():
    """an entry that calls the hook calls it for EVERY index output it has (transpose: t_row_ptrs and
    t_col_idxs), unless the ledger names the parameter: `entry(parameter): reason`"""
    led = ledger()
    bad = []
    for path in sorted(CSRC.glob("*.hip")):
        for name, stem, params, body in definitions(path):
            if HOOK not in body:
                continue
            told = set(re.findall(HOOK + r"\(\s*(\w+)", body))
            for out in index_outputs(params):
                if out not in told and "%s(%s)" % (stem, out) not in led:
                    bad.append("%s: %s(%s)" % (path.name, name, out))
    assert not bad, bad


def test_ledger_is_exact():
    found, led = scan(), ledger()
    for name, reason in led.items():
        stem = name.split("(")[0]
        assert stem in found, "the ledger names %s, which no source file defines with an index output" % stem
        assert len(reason) >= 12, "no reason for %s" % name
        if "(" not in name:
            assert not found[stem]["hooked"], "%s calls the hook: delete its line from the ledger" % stem
        else:
            assert name[len(stem) + 1:-1] in found[stem]["outputs"], name


def test_header_names_the_hooked_entries():
    found = scan()
    hooked = {s for s, e in found.items() if e["some_hooked"]} - {"gkoc_csr_structure_changed"}
    entries = [e for e in header_names() if e != {"gkoc_csr_structure_changed"}]
    named = set().union(*entries)
    assert {"gkoc_free", "gkoc_memcpy_h2d", "gkoc_memcpy_d2d", "gkoc_memset", "gkoc_csr_transpose"} <= named
    assert not hooked - named, "hooked, not in the header's contract: %s" % sorted(hooked - named)
    ghosts = [sorted(e) for e in entries if not e & hooked]
    assert not ghosts, "in the header's contract, no such entry calls the hook: %s" % ghosts
    # [_optional] spellings: where both exist (gkoc_csr_submatrix[_from_index_set]) both are hooked
    for e in entries:
        for name in e - hooked:
            assert name not in found, "%s writes an index array and is named by the header, without the hook" % name
