"""Host side of the PFD path (no GPU): a fold shape the library refuses fails its own folds,
with the library's message, and every other shape group of the batch is still scored."""
import numpy as np

from pulsarfeatureextractor_amd import processor
from pulsarfeatureextractor_amd._native import PFE_PFD_NDM, PfeError
from pulsarfeatureextractor_amd.synth import pfd_fold_block

BAD = (5, 24)  # (nsub, proflen) the stub refuses
MSG = "pfd stub: nsub=5 proflen=24 unsupported"


class StubEngine:
    """pfd_dmprof / pfd_bates22 that raise for one shape and return values that name the fold
    (its profs sum) otherwise."""

    def __init__(self):
        self.calls = []

    def _tag(self, fn, profs):
        n, _npart, nsub, L = profs.shape
        self.calls.append((fn, nsub, L, n))
        if (nsub, L) == BAD:
            raise PfeError(MSG)
        return profs.reshape(n, -1).sum(axis=1)

    def pfd_dmprof(self, profs, subfreqs, scal, profile=True, chis=True, lyon8=True):
        t = self._tag("pfd_dmprof", profs)
        n, L = profs.shape[0], profs.shape[3]
        return {"profile": t[:, None] + np.arange(L)[None, :] if profile else None,
                "chis": (t[:, None] + np.arange(PFE_PFD_NDM)[None, :]).astype(np.float32) if chis else None,
                "lyon8": t[:, None] + np.arange(8)[None, :] if lyon8 else None,
                "status": np.zeros(n, dtype=np.uint32)}

    def pfd_bates22(self, profs, subfreqs, scal, out=None, status=None):
        t = self._tag("pfd_bates22", profs)
        return t[:, None] + np.arange(22)[None, :], np.zeros(profs.shape[0], dtype=np.uint32)


def batch():
    """Good and refused folds interleaved: [good, bad, good, bad, good]."""
    good = pfd_fold_block(3, (2, 4, 16), 11)
    bad = pfd_fold_block(2, (2,) + BAD, 23)
    datas = [good[0], bad[0], good[1], bad[1], good[2]]
    return datas, [0, 2, 4], [1, 3]


def tag(d):
    return d.profs.sum()


def test_score_pfd_refused_shape_fails_alone():
    datas, good, bad = batch()
    eng = StubEngine()
    out, profiles, err = processor.score_pfd(datas, eng)
    for i in bad:
        assert MSG in err[i]
        assert np.isnan(out[i]).all() and profiles[i] is None
    for i in good:
        assert err[i] is None
        assert np.allclose(out[i], tag(datas[i]) + np.arange(8))
        assert np.allclose(profiles[i], tag(datas[i]) + np.arange(16))
    assert {c[1:3] for c in eng.calls} == {(4, 16), BAD}


def test_score_pfd22_refused_shape_fails_alone():
    datas, good, bad = batch()
    out, err = processor.score_pfd22(datas, StubEngine())
    for i in bad:
        assert MSG in err[i]
        assert np.isnan(out[i]).all()
    for i in good:
        assert err[i] is None
        assert np.allclose(out[i], tag(datas[i]) + np.arange(22))


def test_pfd_profile_and_curve_refused_shape_fails_alone():
    datas, good, bad = batch()
    profiles, curves, err = processor.pfd_profile_and_curve(datas, StubEngine())
    for i in bad:
        assert MSG in err[i]
        assert profiles[i] is None and curves[i] is None
    for i in good:
        assert err[i] is None
        assert np.allclose(profiles[i], tag(datas[i]) + np.arange(16))
        assert curves[i].dtype == np.float32 and len(curves[i]) == PFE_PFD_NDM
