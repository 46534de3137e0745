"""The build entry rebuilds the library when any header of csrc changes: its header list is the directory, not a hand-kept list."""
import os

import __graft_entry__ as g


def test_headers_hold_every_hpp_of_csrc():
    assert g.HEADERS == sorted(f for f in os.listdir(g.CSRC) if f.endswith(".hpp"))
    assert {"das_simple.hpp", "das_krylov.hpp", "das_krylov_debug.hpp", "das_bilu_debug.hpp"} <= set(g.HEADERS)
