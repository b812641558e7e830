"""Host side of the kill masks: pfd.varprof against the reference's double loop (calc_varprof,
PFDFile.py:320-326) on random masks, show_pfd's list syntax, pfd.kill_masks, the attributes
pfd.read sets, the command line's usage errors, and the run's kill lists on the parsed path of
the processor under an engine that is not libpfe's (it gets a zapped copy and complete scal)."""
import numpy as np
import pytest

from pulsarfeatureextractor_amd import cli, pfd, processor
from pulsarfeatureextractor_amd._native import PfeError
from pulsarfeatureextractor_amd.synth import pfd_candidate


def calc_varprof(stats, killed_intervals, killed_subbands):
    """PFDFile.calc_varprof (:314-326), as the reference writes it."""
    varprof = 0.0
    for part in range(stats.shape[0]):
        if part in killed_intervals:
            continue
        for sub in range(stats.shape[1]):
            if sub in killed_subbands:
                continue
            varprof += stats[part][sub][5]
    return varprof


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def test_varprof_is_the_double_loop():
    rng = np.random.default_rng(20261021)
    for _ in range(200):
        npart, nsub = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        stats = rng.normal(size=(npart, nsub, 7)) * 10.0 ** rng.integers(-3, 8)
        kp, ks = rng.random(npart) < 0.3, rng.random(nsub) < 0.3
        want = calc_varprof(stats, list(np.flatnonzero(kp)), list(np.flatnonzero(ks)))
        assert bits(pfd.varprof(stats[:, :, 5], kp, ks)) == bits(want)
        assert bits(pfd.varprof(stats[:, :, 5], kp.astype(np.uint8), None)) == bits(
            calc_varprof(stats, list(np.flatnonzero(kp)), []))
    # a batch, masks per fold and one mask for all; nothing killed is the plain sum in order
    v = rng.normal(size=(5, 4, 6))
    kp, ks = rng.random((5, 4)) < 0.4, rng.random((5, 6)) < 0.4
    got = pfd.varprof(v, kp, ks)
    assert got.shape == (5,)
    for i in range(5):
        assert bits(got[i]) == bits(pfd.varprof(v[i], kp[i], ks[i]))
        assert bits(pfd.varprof(v, kp[0], ks[0])[i]) == bits(pfd.varprof(v[i], kp[0], ks[0]))
    s = np.zeros((4, 6, 7))
    s[:, :, 5] = v[0]
    assert bits(pfd.varprof(v[0])) == bits(calc_varprof(s, [], []))
    # every row killed, and a first term of -0.0: the loop starts from +0.0
    assert bits(pfd.varprof(v[0], np.ones(4, bool))) == bits(0.0)
    assert bits(pfd.varprof(np.full((1, 1), -0.0))) == bits(0.0)


def test_list_parser():
    assert pfd.parse_kill_list("0,3:5") == [0, 3, 4, 5]
    assert pfd.parse_kill_list("7") == [7]
    assert pfd.parse_kill_list("2:2, 0") == [2, 0]
    assert pfd.parse_kill_list("") == []
    for bad in ("a", "1:", "5:3", "-1", "1:2:3", "1.5"):
        with pytest.raises(ValueError):
            pfd.parse_kill_list(bad)


def test_read_sets_the_kill_lists_and_keeps_stats(tmp_path):
    c = pfd_candidate(np.random.default_rng(3), 4, 6, 32)
    p = str(tmp_path / "a.pfd")
    pfd.write(p, **c)
    d = pfd.read(p)
    assert d.killed_intervals == [] and d.killed_subbands == []
    assert d.killed_intervals is not d.killed_subbands
    assert np.array_equal(d.stats, c["stats"])
    assert bits(d.varprof) == bits(pfd.varprof(d.stats[:, :, 5]))
    profs, subfreqs, scal = pfd.batch_inputs([d])   # signature and return value as before
    assert profs.shape == (1, 4, 6, 32) and subfreqs.shape == (1, 6) and scal.shape == (1, 8)


def test_kill_masks():
    mk = lambda ki, ks: pfd.PFDData(npart=4, nsub=6, killed_intervals=ki, killed_subbands=ks)  # noqa: E731
    assert pfd.kill_masks([mk([], []), mk([], [])]) == (None, None)
    assert pfd.kill_masks([pfd.PFDData(npart=4, nsub=6)]) == (None, None)
    parts, subs = pfd.kill_masks([mk([], []), mk([0, 3], [5]), mk([], [1, 2])])
    assert parts.dtype == subs.dtype == np.uint8
    assert parts.tolist() == [[0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0]]
    assert subs.tolist() == [[0] * 6, [0, 0, 0, 0, 0, 1], [0, 1, 1, 0, 0, 0]]


def test_cli_usage_errors(tmp_path, monkeypatch, capsys):
    """--killsubs / --killparts are valid with --pfd only, and a list must parse: usage errors,
    before any output file is made."""
    monkeypatch.chdir(tmp_path)
    for argv in (["--phcx", "--killsubs", "1"], ["--killparts", "0"], ["--pfd", "--phcx", "--killsubs", "1"],
                 ["--superb", "--killparts", "0:2"], ["--pfd", "--killsubs", "x"],
                 ["--pfd", "--killparts", "3:1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-c", str(tmp_path), "-o", "out.csv", *argv])
        assert e.value.code == 2
        assert "--kill" in capsys.readouterr().err
    assert not (tmp_path / "out.csv").exists()


class _Spy:
    """An engine that is not libpfe's: it records what it is given."""

    def pfd_dmprof(self, profs, subfreqs, scal, **kw):
        self.seen = (profs, subfreqs, scal, kw)
        return "r"


def test_processor_kill_lists_on_parsed_folds(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # (a DataProcessor makes its error log where it is)
    datas = []
    for i in range(3):
        c = pfd_candidate(np.random.default_rng(10 + i), 4, 6, 32)
        datas.append(pfd.PFDData(npart=4, nsub=6, proflen=32, profs=c["profs"], stats=c["stats"],
                                 bestdm=c["bestdm"], binspersec=1.0, avgprof=None, varprof=1.0,
                                 dms=c["dms"], numdms=len(c["dms"]), bary_p1=1.0,
                                 subfreqs=np.arange(6.0)))
    eng = _Spy()
    assert processor._pfd_call(eng, "pfd_dmprof", datas, ([1, 4], [0])) == "r"
    profs, _fr, scal, kw = eng.seen
    assert kw == {}
    for i, d in enumerate(datas):
        z = np.array(d.profs)
        z[0] = 0.0
        z[:, [1, 4]] = 0.0
        assert np.array_equal(profs[i], z)
        assert bits(scal[i, 2]) == bits((z / 32).sum())
        kp, ks = np.zeros(4, bool), np.zeros(6, bool)
        kp[0] = ks[1] = ks[4] = True
        assert bits(scal[i, 3]) == bits(pfd.varprof(d.stats[:, :, 5], kp, ks))
        assert d.profs[0].any()     # the fold's own cube is not modified
    with pytest.raises(PfeError, match="sub-band 6 out of range"):
        processor._pfd_call(eng, "pfd_dmprof", datas, ([6], []))
    with pytest.raises(PfeError, match="interval 4 out of range"):
        processor._pfd_call(eng, "pfd_dmprof", datas, ([], [4]))
    assert processor._kill_masks(None, 4, 6) == {} and processor._kill_masks(([], []), 4, 6) == {}
    dp = processor.DataProcessor(engine=eng, log=lambda *a: None, kill_subbands=[1], kill_intervals=[0, 2])
    assert dp._kill() == ([1], [0, 2])
    assert processor.DataProcessor(engine=eng, log=lambda *a: None)._kill() is None


class _ScoreSpy:
    """Records the PFD calls a PFDFile makes (an engine that is not libpfe's)."""

    def __init__(self):
        self.calls = []

    def pfd_bates22(self, profs, subfreqs, scal, **kw):
        self.calls.append((np.array(scal), kw))
        return np.zeros((1, 22)), np.zeros(1, dtype=np.uint32)


def test_empty_kill_lists_change_nothing(tmp_path):
    """kill_intervals([]) / kill_subbands([]) on a fold with nothing killed (an RFI finder that
    found nothing) leave every later score as it was: the average is kept, the plain call runs."""
    from pulsarfeatureextractor_amd.candidate import PFDFile

    p = str(tmp_path / "a.pfd")
    pfd.write(p, **pfd_candidate(np.random.default_rng(5), 4, 6, 32))
    eng = _ScoreSpy()
    f = PFDFile(False, p, engine=eng)
    f.compute()
    f.kill_intervals([])
    f.kill_subbands([])
    assert f.killed_intervals == [] and f.killed_subbands == []
    f.compute()
    (before, kw0), (after, kw1) = eng.calls
    assert kw0 == kw1 == {}
    assert np.isfinite(before[0, 2]) and bits(before) == bits(after)
    # with something killed the average is derived from the zapped cube; an empty list after
    # that changes nothing either
    f.kill_subbands([2])
    f.kill_intervals([])
    f.compute()
    _scal, kw = eng.calls[-1]
    assert kw["derive_avgprof"] is True and kw["kill_subs"].tolist() == [[0, 0, 1, 0, 0, 0]]
    assert bits(f.data.varprof) == bits(f.calc_varprof())
    # a fold read without its average has the device derive it, masks or not
    d = pfd.read(p, avgprof=False)
    assert f.profileOps._kill(d) == {"derive_avgprof": True}
    assert f.profileOps._kill(pfd.read(p)) == {}


def test_masks_with_a_cube_that_is_not_4d():
    """The method's own ValueError, not an unpacking error, and before any library call."""
    from pulsarfeatureextractor_amd._native import Engine

    e = object.__new__(Engine)   # no handle: _pfd_kill validates before it needs one
    for cube in (np.zeros((3, 4, 5)), np.zeros((2, 3, 4, 5, 6))):
        with pytest.raises(ValueError, match=r"pfd_bates22: profs must be \(n,npart,nsub,L\)"):
            e._pfd_kill("pfd_bates22", cube, np.zeros(3, bool), None)


def test_kill_lists_are_for_pfd_runs(tmp_path, monkeypatch):
    """DataProcessor(kill_subbands=, kill_intervals=) in a run that is not a PFD run is an error
    of the Python API as it is a usage error of the command line."""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "c").mkdir()
    mk = lambda **kw: processor.DataProcessor(engine=_Spy(), log=lambda *a: None, **kw)  # noqa: E731
    out = str(tmp_path / "o.csv")
    with pytest.raises(ValueError, match="PFD runs only"):
        mk(kill_subbands=[1]).processPHCXCollectively(str(tmp_path / "c") + "/", False, out, False, False, False)
    with pytest.raises(ValueError, match="PFD runs only"):
        mk(kill_intervals=[0]).dmprofSUPERB(str(tmp_path / "c") + "/", False, out, False, False)
    with pytest.raises(ValueError, match="PFD runs only"):
        mk(kill_intervals=[0]).processPFDAndPHCXCollectively(str(tmp_path / "c") + "/", False, out, False,
                                                             False, False)
    # a PFD run over an empty directory, and any run without lists, go through
    mk(kill_subbands=[1]).dmprofPFD(str(tmp_path / "c") + "/", False, out, False, False)
    mk().dmprofPHCX(str(tmp_path / "c") + "/", False, out, False, False)
