"""The native .pfd reader (csrc/pfd_io.cpp: pfe_pfd_scan / _info_all / _fetch / _pack) against
the Python reader it stands in for on the batched path: pfd.read and pfd.batch_inputs, code this
reader does not touch.  Every comparison is exact: ints and byte strings equal, every float
compared as its bits.  Files are written by pfd.write and then cut where a case needs it.
CPU only."""
import os
import struct

import numpy as np
import pytest

from pulsarfeatureextractor_amd import _native
from pulsarfeatureextractor_amd import pfd as P

SHAPES = [(1, 1, 2), (3, 5, 7), (8, 16, 64)]
FLOAT_ATTRS = ("dt", "startT", "endT", "tepoch", "bepoch", "avgvoverc", "lofreq", "chan_wid",
               "bestdm", "topo_p1", "bary_p1", "fold_p1", "binspersec", "subdeltafreq",
               "losubfreq", "varprof")
INT_ATTRS = ("numdms", "numperiods", "numpdots", "nsub", "npart", "proflen", "numchan",
             "chanpersub")
BYTES_ATTRS = ("filenm", "candnm", "telescope", "pgdev", "rastr", "decstr")
ARRAY_ATTRS = ("dms", "periods", "pdots", "profs", "stats", "subfreqs")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def spread_stats(rng, npart, nsub):
    """foldstats whose prof_var column spans 1e-8 .. 1e8 with both signs, so that the order of
    the additions shows in the last bits of the sum."""
    st = rng.standard_normal((npart, nsub, 7))
    st[:, :, 5] = rng.standard_normal((npart, nsub)) * 10.0 ** rng.uniform(-8, 8, (npart, nsub))
    return st


def write_file(path, shape, seed=0, big_endian=False, with_posn=True, numdms=100):
    rng = np.random.default_rng(seed)
    npart, nsub, proflen = shape
    P.write(path, profs=rng.standard_normal(shape) * 37.0 + 11.0,
            stats=spread_stats(rng, npart, nsub), dms=np.linspace(3.25, 91.5, numdms),
            bestdm=41.37, fold_p1=0.0123456789, bary_p1=0.0123456701, lofreq=1182.1953125,
            chan_wid=0.390625, numchan=nsub * 4 + 3, big_endian=big_endian, with_posn=with_posn,
            periods=np.linspace(0.0123, 0.0124, 5), pdots=np.linspace(-1e-12, 1e-12, 3))
    return path


def cube_span(path, shape):
    """(offset, bytes) of the cube in a complete file written by write_file."""
    npart, nsub, proflen = shape
    nb = 8 * npart * nsub * proflen
    return os.path.getsize(path) - 56 * npart * nsub - nb, nb


def cut(path, size):
    with open(path, "r+b") as f:
        f.truncate(size)


def assert_same(d, want):
    """Every attribute pfd.read sets (avgprof aside: read with avgprof=False)."""
    assert set(vars(want)) == set(vars(d))
    assert d.swap == want.swap
    for k in INT_ATTRS:
        assert getattr(d, k) == getattr(want, k), k
    for k in BYTES_ATTRS:
        assert getattr(d, k) == getattr(want, k), k
    for k in FLOAT_ATTRS:
        assert bits(getattr(d, k)) == bits(getattr(want, k)), k
    assert len(d.orb) == 7 and (bits(d.orb) == bits(want.orb)).all()
    for k in ARRAY_ATTRS:
        a, b = getattr(d, k), getattr(want, k)
        assert a.shape == b.shape and a.dtype == np.float64 and (bits(a) == bits(b)).all(), k
    assert d.avgprof is None and want.avgprof is None


def python_varprof(stats):
    v = 0.0
    for part in range(stats.shape[0]):
        for sub in range(stats.shape[1]):
            v += stats[part][sub][5]
    return v


@pytest.mark.parametrize("numdms", [1, 100])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_posn", [True, False])
@pytest.mark.parametrize("big_endian", [False, True])
def test_reader_matches_pfd_read(tmp_path, big_endian, with_posn, shape, numdms):
    p = write_file(str(tmp_path / "a.pfd"), shape, seed=7, big_endian=big_endian,
                   with_posn=with_posn, numdms=numdms)
    b = _native.PfdBatch([p], threads=1)
    inf = b.infos()
    assert inf["status"][0] == 0 and inf["big_endian"][0] == big_endian
    assert inf["has_posn"][0] == with_posn
    assert inf["rows"][0] == inf["stat_rows"][0] == shape[0] * shape[1]
    assert inf["cube_off"][0] == cube_span(p, shape)[0]
    want = P.read(p, avgprof=False)
    assert_same(b.data(0), want)
    # the order of the additions matters for these stats: the sum is the sequential one
    assert bits(inf["scal"][0][3]) == bits(python_varprof(want.stats))
    if shape == (8, 16, 64):  # 128 values: numpy's pairwise order gives other bits
        assert bits(inf["scal"][0][3]) != bits(want.stats[:, :, 5].sum())
    b.close()


def cut_cases(tmp_path, big_endian=False):
    """name -> (path, shape) of files cut short in the cube or the foldstats."""
    shape = (3, 5, 7)
    out = {}
    for name in ("mid_row", "row_boundary", "in_stats", "first_row", "no_stats"):
        p = write_file(str(tmp_path / f"{name}_{int(big_endian)}.pfd"), shape, seed=3,
                       big_endian=big_endian)
        off, nb = cube_span(p, shape)
        cut(p, {"mid_row": off + 8 * (7 * 6 + 3), "row_boundary": off + 8 * 7 * 9,
                "in_stats": off + nb + 56 * 4 + 17, "first_row": off + 11,
                "no_stats": off + nb}[name])
        out[name] = (p, shape)
    return out


@pytest.mark.parametrize("name", ["mid_row", "row_boundary", "in_stats", "first_row", "no_stats"])
def test_little_endian_file_cut_short(tmp_path, name):
    p, shape = cut_cases(tmp_path)[name]
    b = _native.PfdBatch([p], threads=1)
    inf = b.infos()[0]
    assert inf["status"] == 0
    want = P.read(p, avgprof=False)
    assert_same(b.data(0), want)
    rows = {"mid_row": 6, "row_boundary": 9, "first_row": 0}.get(name, 15)
    assert inf["rows"] == rows and inf["stat_rows"] == (4 if name == "in_stats" else 0)
    assert (want.profs.reshape(-1, 7)[rows:] == 0).all()  # zeros where pfd.read has zeros
    if rows:
        assert (want.profs.reshape(-1, 7)[:rows] != 0).all()
    b.close()


def failing_files(tmp_path):
    """[(path, expected status name, exception type pfd.read raises)]."""
    shape = (3, 5, 7)
    be_cube = write_file(str(tmp_path / "be_cube.pfd"), shape, big_endian=True)
    off, nb = cube_span(be_cube, shape)
    cut(be_cube, off + nb - 8)
    head = write_file(str(tmp_path / "head.pfd"), shape)
    cut(head, 150)
    head_be = write_file(str(tmp_path / "head_be.pfd"), shape, big_endian=True)
    cut(head_be, cube_span(head_be, shape)[0] - 9)  # inside pdots
    tiny = write_file(str(tmp_path / "tiny.pfd"), shape)
    cut(tiny, 19)
    empty = str(tmp_path / "empty.pfd")
    open(empty, "wb").close()
    return [(be_cube, "cube", struct.error), (head, "header", struct.error),
            (head_be, "header", struct.error), (tiny, "header", struct.error),
            (empty, "header", struct.error),
            (str(tmp_path / "missing.pfd"), "open", FileNotFoundError),
            (str(tmp_path), "open", IsADirectoryError)]


def test_files_the_reader_hands_back(tmp_path):
    cases = failing_files(tmp_path)
    good = write_file(str(tmp_path / "good.pfd"), (3, 5, 7))
    b = _native.PfdBatch([c[0] for c in cases] + [good], threads=4)
    inf = b.infos()
    for k, (path, status, exc) in enumerate(cases):
        assert _native.PFE_IO_STATUS[int(inf["status"][k])] == status, path
        with pytest.raises(exc):  # the fallback raises what it always raised
            P.read(path, avgprof=False)
        with pytest.raises(_native.PfeError):
            b.fetch(k, _native.PFE_PFD_F_DMS, 100)
        with pytest.raises(_native.PfeError):
            b.pack([k], (3, 5, 7))
    assert inf["status"][-1] == 0
    b.close()


def test_header_counts_the_reader_does_not_take_on(tmp_path):
    p = write_file(str(tmp_path / "a.pfd"), (3, 5, 7))
    raw = bytearray(open(p, "rb").read())
    raw[0:4] = struct.pack("<i", 0)  # numdms = 0: batch_inputs cannot take dms[0]
    q = str(tmp_path / "nodms.pfd")
    open(q, "wb").write(bytes(raw))
    raw = bytearray(open(p, "rb").read())
    raw[48:52] = struct.pack("<i", -3)  # a negative string length
    r = str(tmp_path / "neglen.pfd")
    open(r, "wb").write(bytes(raw))
    b = _native.PfdBatch([q, r])
    assert [_native.PFE_IO_STATUS[int(s)] for s in b.infos()["status"]] == ["value", "value"]
    b.close()


def group_files(tmp_path, big_endian, n=5, shape=(3, 5, 7)):
    return [write_file(str(tmp_path / f"g{int(big_endian)}_{k}.pfd"), shape, seed=20 + k,
                       big_endian=big_endian, numdms=1 if k == 2 else 100) for k in range(n)]


@pytest.mark.parametrize("big_endian", [False, True])
def test_pack_matches_file_bytes_and_batch_inputs(tmp_path, big_endian):
    shape = (3, 5, 7)
    paths = group_files(tmp_path, big_endian)
    spans = [cube_span(p, shape) for p in paths]
    if not big_endian:  # a cube cut short packs as zeros from the first incomplete row on
        cut(paths[3], spans[3][0] + 8 * (7 * 4 + 2))
    rows = [4, 0, 3, 1, 2]
    slabs = []
    for threads in (1, 4):
        b = _native.PfdBatch(paths, threads=threads)
        a = b.pack(rows, shape, threads=threads)
        b.close()
        slabs.append(a)
        for j, k in enumerate(rows):
            off, nb = spans[k]
            raw = open(paths[k], "rb").read()[off:off + nb]
            if k == 3 and not big_endian:
                raw = raw[:8 * 7 * 4].ljust(nb, b"\0")
            assert a["profs"][j].tobytes() == raw
    for k in ("profs", "subfreqs", "scal"):
        assert slabs[0][k].tobytes() == slabs[1][k].tobytes()
    datas = [P.read(paths[k], avgprof=False) for k in rows]
    profs, subfreqs, scal = P.batch_inputs(datas)
    a = slabs[0]
    cube = a["profs"].byteswap() if big_endian else a["profs"]
    assert (bits(cube) == bits(profs)).all()
    assert (bits(a["subfreqs"]) == bits(subfreqs)).all()
    keep = [c for c in range(8) if c != _native.PFE_PFD_AVGPROF]
    assert (bits(a["scal"][:, keep]) == bits(scal[:, keep])).all()
    assert np.isnan(a["scal"][:, _native.PFE_PFD_AVGPROF]).all()
    assert np.isnan(scal[:, _native.PFE_PFD_AVGPROF]).all()  # read with avgprof=False


def test_pack_refuses_mixed_rows(tmp_path):
    le = write_file(str(tmp_path / "le.pfd"), (3, 5, 7))
    be = write_file(str(tmp_path / "be.pfd"), (3, 5, 7), big_endian=True)
    other = write_file(str(tmp_path / "other.pfd"), (5, 3, 7))  # as many values, another shape
    b = _native.PfdBatch([le, be, other])
    lib = _native.load_library()
    dst = np.empty((2, 3, 5, 7))
    sf, sc = np.empty((2, 5)), np.empty((2, 8))

    def raw_pack(rows):
        r = np.asarray(rows, dtype=np.int64)
        return lib.pfe_pfd_pack(b._h, r.ctypes.data, len(r), 1, dst.ctypes.data, sf.ctypes.data,
                                sc.ctypes.data)

    assert raw_pack([0, 0]) == _native.PFE_OK
    assert raw_pack([0, 1]) != _native.PFE_OK   # mixed byte orders
    assert raw_pack([0, 2]) != _native.PFE_OK   # mixed shapes
    assert raw_pack([0, 3]) != _native.PFE_OK and raw_pack([-1]) != _native.PFE_OK
    with pytest.raises(_native.PfeError):
        b.pack([0, 1], (3, 5, 7))
    with pytest.raises(_native.PfeError):
        b.pack([0], (3, 5, 8))  # the destination is sized by the shape: it must be the file's
    b.close()


def test_default_thread_count_is_bounded(tmp_path):
    """nthreads <= 0 scans and packs as any other count does (16 threads at the most)."""
    paths = group_files(tmp_path, False, n=3)
    a = _native.PfdBatch(paths, threads=0)
    b = _native.PfdBatch(paths, threads=1)
    assert a.infos().tobytes() == b.infos().tobytes()
    assert a.pack([0, 1, 2], (3, 5, 7), threads=-1)["profs"].tobytes() == \
        b.pack([0, 1, 2], (3, 5, 7), threads=1)["profs"].tobytes()
