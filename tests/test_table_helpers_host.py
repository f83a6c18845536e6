"""grafimo_amd.graph_tables without a GPU: the width groups, where a table's file goes and the wide-matrix writer."""
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from grafimo_amd import graph_tables as gt  # noqa: E402
from grafimo_amd.res_writer import DEFAULT_OUTDIR  # noqa: E402


class _Out:
    def __init__(self, outdir):
        self.outdir = outdir


class _Motif:
    motif_id = "MA1.1"

    def __init__(self, width=0):
        self.width = width


def test_group_by_width_keeps_first_seen_order():
    motifs = [_Motif(w) for w in (15, 8, np.int64(15), 19, 8)]
    by_width = gt.group_by_width(motifs)
    assert list(by_width.items()) == [(15, [0, 2]), (8, [1, 4]), (19, [3])]
    assert all(type(w) is int for w in by_width)
    assert gt.group_by_width([]) == {}


def test_table_path(tmp_path, monkeypatch):
    """the rule the six writers and write_results share: the user's directory with the stem, the motif's id behind it
    when several motifs share that directory; the default directory named after the pid and the motif -- or the tag of a
    table made once per call -- with the bare stem"""
    o = _Out(str(tmp_path / "o"))
    assert gt.table_path("grafimo_x", o, _Motif(), 1) == str(tmp_path / "o" / "grafimo_x.tsv") and os.path.isdir(o.outdir)
    assert gt.table_path("grafimo_x", o, _Motif(), 2) == str(tmp_path / "o" / "grafimo_x_MA1.1.tsv")
    assert gt.table_path("grafimo_x", o, tag="pairs") == str(tmp_path / "o" / "grafimo_x.tsv")
    monkeypatch.chdir(tmp_path)
    dflt = gt.table_path("grafimo_x", _Out(DEFAULT_OUTDIR), _Motif(), 2)
    assert dflt == os.path.join(f"grafimo_out_{os.getpid()}_MA1.1", "grafimo_x.tsv") and os.path.isdir(os.path.dirname(dflt))
    assert gt.table_path("grafimo_x", object(), _Motif(), 2) == dflt              # (no outdir at all: the default one)
    dflt = gt.table_path("grafimo_x", _Out(DEFAULT_OUTDIR), tag="pairs")
    assert dflt == os.path.join(f"grafimo_out_{os.getpid()}_pairs", "grafimo_x.tsv") and os.path.isdir(os.path.dirname(dflt))


def _joined(header, head, names, codes, strings):
    lines = ["\t".join(header)] + [head + name + "\t" + "\t".join(strings[c].decode() for c in row)
                                   for name, row in zip(names, codes.tolist())]
    return ("\n".join(lines) + "\n").encode()


@pytest.mark.parametrize("cell_bytes", [1 << 25, 1])
def test_write_wide_equals_a_plain_join(tmp_path, cell_bytes):
    """a 3 x 2 and a 0-row matrix whose cells include the empty string -- in the last column too, where the line ends --
    to a stream and to a file, whole and a row at a time"""
    strings = [b"", b"7", b"-12.25", b"1e-05"]
    tab, ln = gt.text_table(strings)
    assert tab.shape == (4, 7) and ln.tolist() == [1, 2, 7, 6]
    header, head = ["motif_id", "motif_alt_id", "sequence_name", "a|1", "a|2"], "MA1.1\tONE\t"
    for codes, names in ((np.array([[2, 0], [0, 3], [1, 1]]), ["c:0-10", "c:5-9", "d:1-2"]),
                         (np.zeros((3, 2), np.int32), ["c:0-10", "c:5-9", "d:1-2"]), (np.zeros((0, 2), np.int64), [])):
        names = np.array(names, dtype=object)
        want = _joined(header, head, names, codes, strings)
        buf = io.BytesIO()
        assert gt.write_wide(buf, header, head, names, codes, tab, ln, cell_bytes) is None and buf.getvalue() == want
        path = str(tmp_path / f"wide_{len(names)}.tsv")
        assert gt.write_wide(path, header, head, names, codes, tab, ln, cell_bytes) == path
        assert open(path, "rb").read() == want
    assert not buf.closed and want == b"\t".join(h.encode() for h in header) + b"\n"
