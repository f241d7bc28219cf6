"""nh_overlap_wide and nh_penetration_wide on the host (no GPU): both calls are declared in the header with nh_overlap's and nh_penetration's
arguments, exported by the library and wrapped by the engine; the observers note and the layer-mask contract name them; DESIGN has their section."""
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nudge_amd import engine as E           # noqa: E402

WIDE = ("nh_overlap_wide", "nh_penetration_wide")


def _header():
    return open(os.path.join(ROOT, "include", "nudge_hip.h")).read()


def _flat(text):
    return re.sub(r"\s+", " ", text)


def test_both_calls_are_declared_exported_and_wrapped():
    hdr = _header()
    flat = _flat(re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    protos = {}
    for name, hit in (("nh_overlap", "nh_OverlapHit"), ("nh_penetration", "nh_PenetrationHit")):
        for n in (name, name + "_wide"):
            m = re.search(r"int %s\((.*?)\);" % n, flat)
            assert m, n
            protos[n] = m.group(1)
        # the wide form takes the arguments of the plain one, word for word
        assert protos[name] == protos[name + "_wide"], (protos[name], protos[name + "_wide"])
        assert protos[name] == ("nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets , %s* hits, uint32_t capacity, "
                                "uint32_t flags " % hit)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    for n in WIDE:
        assert n in E.EXPORTS
        assert re.search(r"\bT %s$" % n, syms, flags=re.M), n
    for wide, plain in (("overlap_wide", "overlap"), ("penetration_wide", "penetration"), ("overlap_wide_records", "overlap_records"),
                        ("penetration_wide_records", "penetration_records")):
        assert list(inspect.signature(getattr(E.World, wide)).parameters) == list(inspect.signature(getattr(E.World, plain)).parameters), wide
    # the argtypes are set where the library has the calls (and guarded, so that an older library still loads)
    L = E.lib()
    assert L.nh_overlap_wide.argtypes == L.nh_overlap.argtypes and L.nh_penetration_wide.argtypes == L.nh_penetration.argtypes
    src = inspect.getsource(E.lib)
    assert 'hasattr(L, "nh_overlap_wide")' in src


def test_the_observers_note_and_the_filter_contract_name_them():
    hdr = _header()
    line = [l for l in hdr.split("\n") if "The scene queries (nh_query_build" in l]
    assert len(line) == 1
    for n in WIDE:
        assert n + "," in line[0] or n + ")" in line[0], n
    flat = _flat(hdr)
    a = flat.index("THE CONTRACT, for all twenty-five query calls")
    contract = flat[a:flat.index("Identities that follow", a)]
    assert "twenty-three" not in contract
    for n in WIDE:
        assert n in contract, n
    assert "masks[i] for query i" in contract
    # the calls' own block: nh_overlap's bytes, observers, which call for which size
    b = flat.index("/* nh_overlap_wide and nh_penetration_wide")
    block = flat[b:flat.index("*/", b)]
    for phrase in ("BYTE FOR BYTE", "OBSERVERS", "q_wide_count", "q_wide_list", "DESIGN 10.22", "CALLER CHOOSES THE CALL BY SIZE"):
        assert phrase in block, phrase


def test_the_documents_have_the_section():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "10.22" in design and "nh_overlap_wide" in design and "k_q_wide" in design
    assert "a wave per large query is not built" not in design
    for doc in ("README.md", "INTEGRATION.md", os.path.join("docs", "KERNELS.md"), os.path.join("tools", "README.md")):
        assert "overlap_wide" in open(os.path.join(ROOT, doc)).read(), doc
