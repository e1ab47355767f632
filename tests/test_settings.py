"""The library's environment switches are read in one place (lastz_amd/csrc/lz_settings.hpp; lz_share.hip keeps the four of
the rank protocol), tools/README.md lists exactly those, and the GPU children are scrubbed of names that exist.  Plain
Python over the source text."""
import os
import re

import helpers as H

CSRC = os.path.join(H.ROOT, "lastz_amd", "csrc")
READERS = ("lz_settings.hpp", "lz_share.hip")
GETENV = re.compile(r'getenv\("(LZGPU_[A-Z0-9_]+)"')


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _switches(name):
    """the switches a source file reads: a name counts where it is handed to getenv (lz_share.hip also holds LZGPU_ERR_* codes)"""
    return set(GETENV.findall(_read(name)))


def test_getenv_only_in_the_settings_header_and_the_rank_protocol():
    for f in sorted(os.listdir(CSRC)):
        if f not in READERS:
            assert 'getenv("LZGPU_' not in _read(f), f
    assert len(_switches("lz_settings.hpp")) > 10 and len(_switches("lz_share.hip")) == 4


def test_tools_readme_lists_the_switches_the_library_reads():
    """the list's items headed `Library` against the two files, name for name; the shim's, bench.py's, the tests' and the build's
    names stand under headings of their own and are not compared"""
    text = open(os.path.join(H.ROOT, "tools", "README.md")).read()
    listed = text.split("Developer environment switches", 1)[1]
    items = re.findall(r"^\* ([^:\n]+):(.*?)(?=^\* |\Z)", listed, re.M | re.S)
    library = [body for head, body in items if head.startswith("Library")]
    assert len(library) >= 2 and len(library) < len(items)
    documented = set(re.findall(r"LZGPU_[A-Z0-9_]+", " ".join(library)))
    assert documented == _switches("lz_settings.hpp") | _switches("lz_share.hip")


def test_children_are_scrubbed_of_switches_that_exist():
    assert H.CHILD_SCRUB and set(H.CHILD_SCRUB) <= _switches("lz_settings.hpp")
