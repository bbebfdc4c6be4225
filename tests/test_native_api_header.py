"""csrc/api.h is the one description of the native boundary: every
extern "C" launcher a .hip defines is declared there (the compilers check
a definition against a prototype they see, but accept one with none),
every declared launcher is defined exactly once, and bind.cpp declares
nothing of its own.  A text scan, no build."""

import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "bdbnn_amd", "csrc")


def _read(path):
    with open(path) as f:
        return f.read()


def _sources(pattern):
    """committed sources only: hipify leaves *_hip.* copies beside them"""
    return [p for p in sorted(glob.glob(os.path.join(CSRC, pattern)))
            if not re.search(r"_hip\.\w+$", p)]


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _defined():
    """{name: [files]} of extern "C" ... bdbnn_*( in the .hip sources"""
    out = {}
    for path in _sources("*.hip"):
        text = _strip_comments(_read(path))
        for m in re.finditer(r'extern\s+"C"\s+[\w\s\*]*?\b(bdbnn_\w+)\s*\(',
                             text):
            out.setdefault(m.group(1), []).append(os.path.basename(path))
    return out


def _declared():
    text = _strip_comments(_read(os.path.join(CSRC, "api.h")))
    m = re.search(r'extern\s+"C"\s*\{(.*)\}', text, flags=re.S)
    assert m, 'api.h has no extern "C" { } block'
    assert len(re.findall(r'extern\s+"C"', text)) == 1
    names = re.findall(r"\b(bdbnn_\w+)\s*\(", m.group(1))
    assert len(names) == len(set(names)), "a launcher is declared twice"
    return set(names)


def test_every_defined_launcher_is_declared():
    defined = _defined()
    assert len(defined) > 50, "the scan found too few launchers"
    missing = sorted(set(defined) - _declared())
    assert not missing, f"defined in a .hip, not declared in api.h: {missing}"


def test_every_declared_launcher_is_defined_once():
    defined = _defined()
    wrong = {n: defined.get(n, []) for n in sorted(_declared())
             if len(defined.get(n, [])) != 1}
    assert not wrong, f"declared in api.h, not defined exactly once: {wrong}"


def test_bind_declares_nothing_itself():
    text = _strip_comments(_read(os.path.join(CSRC, "bind.cpp")))
    assert 'extern "C"' not in text
    assert re.search(r'#include\s+"api\.h"', text)


def test_shared_structs_occur_once():
    text = "\n".join(_strip_comments(_read(p))
                     for pat in ("*.hip", "*.h", "*.cpp")
                     for p in _sources(pat))
    assert len(re.findall(r"\bstruct\s+TensorListArg\b\s*\{", text)) == 1
    ptr_list = re.findall(
        r"\bstruct\s+\w+\s*\{\s*float\s*\*\s*ptr\s*\[\s*BDBNN_MAX_TENSORS"
        r"\s*\]\s*;\s*\}", text)
    assert len(ptr_list) == 1, ptr_list
