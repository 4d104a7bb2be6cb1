"""Every device buffer of the engine has a row in DESIGN.md's ledger (§7a): who allocates it, what
initialises it, who writes which extent first and why every read stays inside that. A DevArray
member added to rl_engine_impl.hpp without a row fails here. CPU only."""
import os
import re

import rl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPL = os.path.join(rl_amd.PKG_DIR, "csrc", "rl_engine_impl.hpp")
DESIGN = os.path.join(ROOT, "DESIGN.md")
ROUTER = os.path.join(rl_amd.PKG_DIR, "csrc", "rl_router.cpp")


def dev_array_members():
    src = open(IMPL).read()
    src = re.sub(r"//[^\n]*", "", src)
    names = []
    for decl in re.findall(r"\bDevArray<[^;{}()]*>\s+([^;{}()]+);", src):
        names += [n.strip() for n in decl.split(",")]
    return names


def ledger_section():
    text = open(DESIGN).read()
    m = re.search(r"^## 7a\. Device buffers: the ledger\n(.*?)(?=^## )", text, re.S | re.M)
    assert m, "DESIGN.md has no section '7a. Device buffers: the ledger'"
    return m.group(1)


def ledger_rows():
    """name -> the row's cells, for every backticked name in the first cell of a table row."""
    rows = {}
    for line in ledger_section().splitlines():
        if not line.startswith("|") or set(line) <= set("|- "):
            continue
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        for name in re.findall(r"`([A-Za-z_][A-Za-z_0-9]*)`", cells[0]):
            rows[name] = cells
    return rows


def test_the_extraction_sees_the_members():
    names = dev_array_members()
    assert len(names) == len(set(names))
    # members declared alone, in pairs and inside BatchScratch
    for n in ("rec0", "rec1", "pos1", "d_ctl", "hot_summ", "walk_tab", "route_cnt", "s_tokens", "ks_hdr"):
        assert n in names, n
    assert len(names) >= 55


def test_every_dev_array_has_a_row():
    rows = ledger_rows()
    missing = [n for n in dev_array_members() if n not in rows]
    assert not missing, f"no ledger row in DESIGN.md §7a for: {missing}"


def test_rows_are_filled_in():
    for name, cells in ledger_rows().items():
        assert len(cells) >= 5, (name, len(cells))
        assert all(cells[:5]), f"{name}: an empty cell"


def test_tables_and_router_buffers_have_rows():
    sec = ledger_section()
    assert "HostLimiter::table" in sec and "cache_table" in sec
    rows = ledger_rows()
    # the router's device pointers: every member freed by rl_router_destroy
    src = open(ROUTER).read()
    m = re.search(r"void\* bufs\[\] = \{(.*?)\};", src, re.S)
    bufs = re.findall(r"r->(\w+)", m.group(1))
    assert len(bufs) >= 20
    missing = [b for b in bufs if b not in rows]
    assert not missing, f"no ledger row for the router's: {missing}"


def test_no_allocation_bypasses_the_helper():
    """One device allocation call in the engine's sources, in dev_malloc: the fill of
    rl_debug_alloc_fill reaches every buffer. Any hip*Malloc* counts (hipMallocAsync, hipMallocManaged,
    hipExtMallocWithFlags ...) except the pinned host memory of hipHostMalloc."""
    csrc = os.path.join(rl_amd.PKG_DIR, "csrc")
    hits = []
    for f in sorted(os.listdir(csrc)):
        for i, line in enumerate(open(os.path.join(csrc, f)), 1):
            code = line.split("//")[0]
            for m in re.finditer(r"\bhip\w*Malloc\w*\s*\(", code):
                if not m.group(0).startswith("hipHostMalloc"):
                    hits.append(f"{f}:{i}")
    assert len(hits) == 1 and hits[0].startswith("rl_engine.cpp:"), hits
