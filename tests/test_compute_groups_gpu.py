"""The five compute*Scores methods of the candidate file classes (CandidateFileInterface.py:
173-194), called one by one in the reference's order (PHCXFile.py:383-409, PFDFile.py:587-613),
against compute() of another instance of the same file: the same scores bit for bit, and a
candidate the reference raises on raises at the method of its group, with the reference's
text, after the methods before it have appended their columns."""
import numpy as np
import pytest

from golden_util import load
from pulsarfeatureextractor_amd import pfd, phcx
from pulsarfeatureextractor_amd.candidate import PFDFile, PHCXFile, SUPERBPHCXFile
from pulsarfeatureextractor_amd.profile_ops import PFDOperations, PHCXOperations
from test_oracle_pfd import build_files, load_set
from test_phcx_native import _write_golden

pytestmark = pytest.mark.gpu

# method, len(self.scores) after it, the text it raises (PHCXFile.py:470, :543, :585, :629, :668)
ORDER = (("computeSinusoidFittingScores", 4, "Sinusoid fitting exception"),
         ("computeGaussianFittingScores", 11, "Gaussian fitting exception"),
         ("computeCandidateParameterScores", 15, "Candidate parameters exception"),
         ("computeDMCurveFittingScores", 19, "DM curve fitting exception"),
         ("computeSubBandScores", 22, "Subband scoring exception"))


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def by_groups(f):
    """Call the five methods in order -> the text of the one that raised, or None."""
    assert f.scores == []
    for name, upto, text in ORDER:
        before = list(f.scores)
        try:
            getattr(f, name)()
        except Exception as e:  # noqa: BLE001 (the reference raises plain Exception)
            assert type(e) is Exception and str(e) == text, (name, repr(e))
            assert f.scores == before, "a method that raises appends nothing"
            return text
        assert len(f.scores) == upto and all(type(v) is float for v in f.scores), name
    return None


def whole(cls, path, engine):
    try:
        return cls(False, path, engine).compute(), None
    except Exception as e:  # noqa: BLE001
        return None, str(e)


@pytest.mark.parametrize("cls,name,n_ok,n_bad", [(PHCXFile, "bates22_phcx128", 12, 3),
                                                 (SUPERBPHCXFile, "bates22_superb64", 8, 0)])
def test_phcx_groups_equal_compute(engine, tmp_path, cls, name, n_ok, n_bad):
    ok = load(name)["ok"].astype(bool)
    rows = list(np.where(ok)[0][:n_ok]) + list(np.where(~ok)[0][:n_bad])
    paths = _write_golden(tmp_path, name, rows)
    raised = 0
    for p in paths:
        ref, msg = whole(cls, p, engine)
        f = cls(False, p, engine)
        assert isinstance(f.profileOps, PHCXOperations)
        got = by_groups(f)
        assert got == msg, p
        d = f.data
        if msg is None:
            assert np.array_equal(bits(f.scores), bits(ref)), p
        else:
            # the columns of the groups before the failing one, as the whole chain holds them
            raised += 1
            out, _st = engine.bates22(d.profile[None, :].astype(np.uint8),
                                      d.subbands[None].astype(np.uint8), d.dm_curve[None, :],
                                      d.scal[None, :])
            k = len(f.scores)
            assert k in (0, 4, 11, 15, 19)
            assert np.array_equal(bits(f.scores), bits(out[0, :k])), p
        curve = f.getDMPlaneCurveData()
        assert isinstance(curve, list)
        assert np.array_equal(bits(curve), bits(phcx.parse(p, superb=cls.SUPERB).dm_curve))
    assert raised == n_bad, "the candidates the reference raised on raise here"


def test_pfd_groups_equal_compute(engine, tmp_path):
    files = build_files(tmp_path, load_set("pfd_64x16"))[:8]
    ops = PFDOperations(engine=engine)
    scored = 0
    for p in files:
        ref, msg = whole(PFDFile, p, engine)
        f = PFDFile(False, p, engine)
        assert isinstance(f.profileOps, PFDOperations)
        assert by_groups(f) == msg, p
        if msg is not None:
            continue
        scored += 1
        assert np.array_equal(bits(f.scores), bits(ref)), p
        # the reference's call (PFDFile.py:859): the file object and its own profile
        sub = ops.getSubbandParameters(f, f.getProfile())
        assert np.array_equal(bits(sub), bits(ref[19:22])), p
        assert ops.getSubbandParameters(pfd.read(p)) == sub and ops.getSubbandParameters(p) == sub
        other = np.array(f.getProfile(), copy=True)
        other[3] += 1.0
        with pytest.raises(ValueError, match="own profile"):
            ops.getSubbandParameters(f, other)
        chis = ops.getDMCurveData(f)
        assert chis.dtype == np.float32 and chis.shape == (100,)
        norm = ops.getDMCurveDataNormalised(f)
        want = np.float32(255.) / max(chis) * chis
        assert norm.dtype == np.float32
        assert np.array_equal(norm.view(np.int32), want.view(np.int32)), p
    assert scored >= 4
