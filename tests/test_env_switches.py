"""CPU: the FVC_* environment switches named by the tests, by kernels._LAYOUT_ENV and by the sources
must agree (plain text scans, no library load).

A switch counts as read where its quoted name is the first argument of getenv / fvc_env_int (C++) or
os.environ.get (Python). A test that sets a name nothing reads runs its default leg twice and proves
nothing: test_conv_x3_weight_paths_identical did so with FVC_X3_BLDS until it was deleted together with
the experiment kernels behind the RETIRED switches (DESIGN_HISTORY.md keeps their account).

The compile-time -D switches of the conv sources are retired as well: csrc/ has no preprocessor
conditional on an FVC_ name, and build.build() builds the one library."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fastvideocodec_amd")

# switches whose non-default kernel forms were removed: the names must not come back by accident
RETIRED = ("FVC_DECONV_FUSED", "FVC_CONV_BPF", "FVC_CONV_WM4", "FVC_CONV_PIPE", "FVC_CONV_PIPE7", "FVC_CONV_NW",
           "FVC_CONV_WN1", "FVC_CONV_WN2", "FVC_CONV_CC", "FVC_X3_WL", "FVC_X3_WG", "FVC_X3_PRIO", "FVC_X3_BPC",
           "FVC_UP2_NT", "FVC_UP2_PAIR", "FVC_GATHER_TH",
           # compile-time -D switches (and the run-time FVC_WINO_CHUNK), folded to their product values
           "FVC_WINO_PIX", "FVC_WINO_KO", "FVC_WINO_KO_WAIT", "FVC_WINO_ALLNOP", "FVC_UP_KO", "FVC_UP_FORM",
           "FVC_UP_FIRST", "FVC_WR7_KO", "FVC_WR7_SPREAD", "FVC_WR7_SPEC", "FVC_WR7_DIST", "FVC_WR7_Q1GAP",
           "FVC_X3_KO", "FVC_X3_SCHED", "FVC_X3_ACC1", "FVC_X3_TRACE", "FVC_DX_KO", "FVC_STORE_AUX", "FVC_STEM_K7",
           "FVC_WINO_CHUNK")

_READ = re.compile(r'(?:getenv|fvc_env_int|environ\.get)\(\s*"(FVC_[A-Z0-9_]+)"')
# monkeypatch.setenv("NAME", ...), os.environ["NAME"] = ..., and {"NAME": ...} tables fed to setenv
_SET = re.compile(r'(?:setenv\(\s*"(FVC_[A-Z0-9_]+)"|environ\[\s*"(FVC_[A-Z0-9_]+)"\s*\]\s*=[^=]|'
                  r'\{\s*"(FVC_[A-Z0-9_]+)"\s*:)')
_SOURCE_EXT = (".py", ".hip", ".h")


def _files(top, exts=_SOURCE_EXT):
    for d, dirs, names in os.walk(top):
        dirs[:] = [n for n in dirs if n not in ("__pycache__", "build")]
        for n in sorted(names):
            if n.endswith(exts):
                yield os.path.join(d, n)


def _text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _reads(top):
    return {m.group(1) for p in _files(top) for m in _READ.finditer(_text(p))}


def test_switches_set_by_tests_are_read():
    read = _reads(PKG)
    unread = {}
    for p in _files(os.path.join(ROOT, "tests"), (".py",)):
        for m in _SET.finditer(_text(p)):
            name = next(g for g in m.groups() if g)
            if name not in read:
                unread.setdefault(name, set()).add(os.path.relpath(p, ROOT))
    assert not unread, f"tests set switches that no source reads: {unread}"


def test_layout_env_entries_are_read():
    m = re.search(r"^_LAYOUT_ENV = \(([^)]*)\)", _text(os.path.join(PKG, "kernels.py")), re.M)
    layout_env = re.findall(r'"(FVC_[A-Z0-9_]+)"', m.group(1)) if m else []
    assert layout_env, "kernels._LAYOUT_ENV not found"
    read = _reads(os.path.join(PKG, "csrc"))
    missing = [k for k in layout_env if k not in read]
    assert not missing, f"_LAYOUT_ENV names no csrc file reads: {missing}"


def test_retired_switches_stay_gone():
    assert len(set(RETIRED)) == len(RETIRED)
    pat = re.compile(r"\b(" + "|".join(RETIRED) + r")\b")
    me = os.path.abspath(__file__)
    found = {}
    for top in (PKG, os.path.join(ROOT, "tests"), os.path.join(ROOT, "include")):
        for p in _files(top, _SOURCE_EXT + (".json", ".md", ".txt", ".sh", ".c")):
            if os.path.abspath(p) == me:  # this file is the list
                continue
            for m in pat.finditer(_text(p)):
                found.setdefault(m.group(1), set()).add(os.path.relpath(p, ROOT))
    assert not found, f"retired switches named again: {found}"


def test_csrc_has_no_compile_time_switches():
    pat = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b[^\n]*\bFVC_[A-Za-z0-9_]*", re.M)
    found = {os.path.relpath(p, ROOT): [m.group(0).strip() for m in pat.finditer(_text(p))]
             for p in _files(os.path.join(PKG, "csrc"), (".hip", ".h"))}
    found = {p: hits for p, hits in found.items() if hits}
    assert not found, f"preprocessor conditionals on FVC_ names: {found}"


def test_build_takes_force_and_verbose_only():
    from fastvideocodec_amd import build as B
    assert list(inspect.signature(B.build).parameters) == ["force", "verbose"]
