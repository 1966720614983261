"""The library's environment switches live in one header, h-slam_amd/csrc/hs_env.h: no other source calls getenv,
INTEGRATION.md's table lists every switch the header reads, and the switches removed with their A/B paths (DESIGN.md
§"The compile-time switches are gone") are named by no source, test or tool."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h-slam_amd", "csrc")

REMOVED = ("HS_TRK_SOLVE", "HS_TRK_ZC", "HS_TRK_GMIN", "HS_TRK_GRAPH", "HS_LIN_PPW", "HS_LIN8_BLOCKS", "HS_TH_BESIDE",
           "HS_SOLVE_DBG", "HS_ACT_DBG", "HS_ACT_PROF", "HS_REF_TRACE")
KEPT = ("HS_ACC_EXACT", "HS_LIN8", "HS_LIN8_NOFILL", "HS_LIN8_HIST", "HS_TH_MULTI", "HS_GRAPH", "HS_HOST_BREAK",
        "HS_EVENT_TIMING", "HS_TRK_G", "HS_TRK_G_UNCHECKED", "HS_TRK_SPIN", "HS_TRK_NOEVT", "HS_KTRACE")


def _files(top, skip_dirs=()):
    for d, dirs, names in os.walk(top):
        dirs[:] = sorted(x for x in dirs if x != "__pycache__" and os.path.join(d, x) not in skip_dirs)
        for n in sorted(names):
            if not n.endswith((".pyc", ".npy", ".npz", ".bin", ".png")):
                yield os.path.join(d, n)


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def test_only_hs_env_calls_getenv():
    users = [os.path.basename(p) for p in _files(CSRC) if "getenv" in _read(p)]
    assert users == ["hs_env.h"], users


def test_integration_table_lists_every_switch():
    read = set(re.findall(r'"(HS_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "hs_env.h"))))
    assert read == set(KEPT), sorted(read ^ set(KEPT))
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    table = set(re.findall(r"^\s*\|\s*`(HS_[A-Z0-9_]+)`\s*\|", doc, flags=re.M))
    assert read <= table, sorted(read - table)


def test_removed_switches_are_named_nowhere():
    tools = os.path.join(ROOT, "tools")
    me = os.path.abspath(__file__)
    hits = []
    for top, skip in ((CSRC, ()), (os.path.join(ROOT, "tests"), ()), (tools, (os.path.join(tools, "archive"),))):
        for p in _files(top, skip):
            if os.path.abspath(p) == me:
                continue
            txt = _read(p)
            # a kept name may extend a removed one's spelling: match whole names only
            hits += [(os.path.relpath(p, ROOT), n) for n in REMOVED if re.search(r"\b%s\b" % n, txt)]
    assert not hits, hits
