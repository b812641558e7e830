"""Drop-in mirror of the reference's second plug-in class, backed by libpfe's per-group entry
points (include/pfe.h: pfe_sinusoid4, pfe_gauss7, pfe_params4, pfe_dmfit4, pfe_subband3).

Reference classes (PulsarFeatureExtractor/src/) and what replaces them here:
  ProfileOperationsInterface  ProfileOperationsInterface.py:38-130 -> ProfileOperationsInterface
  ProfileOperations           ProfileOperations.py:164-          -> ProfileOperations
                              (getSinusoidFittings :190-376, getGaussianFittings :595-770)
  PHCXOperations              PHCXOperations.py:44-             -> PHCXOperations
                              (getCandidateParameters :81-112, getDMFittings :121-233,
                               getSubbandParameters :305-349)
  PFDOperations               PFDOperations.py:62-466           -> PFDOperations
                              (getCandidateParameters :93-233, getDMCurveData :242-272,
                               getDMFittings :274-393, getSubbandParameters :401-466)

A reference-side subclass that needs one score group (PHCXFile.py:454, :521, :569, :613,
:654 call one method each) binds the matching C-ABI function.  Every method here scores one
candidate (the reference's granularity); the `*_batch` forms take n candidates at once.
Values are the bits of the same group's columns of pfe_bates22 (same kernels); where the
reference raises inside a method, the method raises ``Exception`` with the text PHCXFile
reports for that group (candidate.GROUP_ERRORS).  ProfileOperations and PHCXOperations take
the PHCX byte profiles (integers 0-255); PFDOperations also takes the float 0..255 profile of
a PFD (pfe_sinusoid4_f64 / pfe_gauss7_f64) and scores the fold's own groups through
pfe_pfd_params4 / pfe_pfd_dmfit4 / pfe_pfd_subband3.
"""
from __future__ import annotations

import numpy as np

import math

from . import pfd as _pfd
from . import phcx as _phcx
from ._native import PFE_NSCAL, PFE_ST_PFD_DMCURVE_FAIL, Engine
from .candidate import get_engine, status_error


def _py2div(a, b):
    """Python-2 '/': floor division when both operands are integers (the reference runs under
    Python 2.7)."""
    def integral(v):
        return isinstance(v, (int, np.integer)) or (isinstance(v, np.ndarray) and v.dtype.kind in "iu")

    return a // b if integral(a) and integral(b) else a / b


def _score_at_percentile(data, per):
    """scipy.stats.scoreatpercentile(data, per) with its default 'fraction' interpolation, in
    scipy's own operations: the two neighbours of the fractional index weighted by their
    distance to it."""
    srt = np.sort(np.asarray(data))
    idx = per / 100.0 * (srt.shape[0] - 1)
    i = int(idx)
    if i != idx:
        w = np.array([(i + 1) - idx, idx - i], float)
        return np.add.reduce(srt[i:i + 2] * w) / w.sum()
    return np.add.reduce(srt[i:i + 1] * np.array(1)) / 1.0


class ProfileOperationsInterface:
    """ProfileOperationsInterface.py:38-130: the methods a profile-scoring plug-in provides."""

    def __init__(self, debugFlag=False):
        self.debug = debugFlag

    def getSinusoidFittings(self, profile):
        raise NotImplementedError("Please Implement this method")

    def fitSineSqr(self, yData, maxima):
        raise NotImplementedError("Please Implement this method")

    def getGaussianFittings(self, profile):
        raise NotImplementedError("Please Implement this method")

    def fitGaussian(self, xData, yData):
        raise NotImplementedError("Please Implement this method")

    def fitGaussianFixedWidthBins(self, xData, yData, bins):
        raise NotImplementedError("Please Implement this method")

    def fitGaussianWithBackground(self, xData, yData):
        raise NotImplementedError("Please Implement this method")

    def fitGaussianT1(self, yData):
        raise NotImplementedError("Please Implement this method")

    def fitDoubleGaussianT2(self, yData):
        raise NotImplementedError("Please Implement this method")

    def fitDoubleGaussian(self, yData):
        raise NotImplementedError("Please Implement this method")

    def fitDoubleGaussianWithBackground(self, yData, p0):
        raise NotImplementedError("Please Implement this method")

    def getCandidateParameters(self, profile):
        raise NotImplementedError("Please Implement this method")

    def getDMFittings(self, data):
        raise NotImplementedError("Please Implement this method")

    def getSubbandParameters(self, data=None, profile=None):
        raise NotImplementedError("Please Implement this method")

    # ---- the interface's concrete helpers (:138-207), on the host ------------------------
    def freedmanDiaconisRule(self, data):
        """:138-166 -- the number of histogram bins by the Freedman-Diaconis rule; a bin
        width <= 0 (no interquartile range) falls back to 60."""
        iqr = _score_at_percentile(data, 75) - _score_at_percentile(data, 25)
        binwidth = 2 * iqr * pow(len(data), -0.3333333)
        if binwidth <= 0:
            binwidth = 60
        rnge = max(data) - min(data)
        return int(math.ceil(_py2div(rnge, binwidth)))

    def getDerivative(self, yData):
        """:170-186 -- dy[i] = y[i] - y[i+1], as a list."""
        return [yData[i] - yData[i + 1] for i in range(len(yData) - 1)]

    def scale(self, x, min_, max_, newMin, newMax):
        """:190-207 -- x from [min_, max_] to [newMin, newMax], with the reference's Python-2
        '/': all-integer arguments divide as integers."""
        t = _py2div(x - min_, max_ - min_)
        return (newMin * (1 - t)) + (newMax * t)


def _u8_rows(profile) -> np.ndarray:
    p = np.asarray(profile)
    if p.ndim == 1:
        p = p[None, :]
    if p.size and (p.min() < 0 or p.max() > 255 or not np.array_equal(p, np.round(p))):
        raise TypeError("byte profiles (integers 0-255) expected")
    return p.astype(np.uint8)


def _raise_failed(st) -> None:
    for s in np.atleast_1d(np.asarray(st)):
        msg = status_error(int(s))
        if msg:
            raise Exception(msg)


class ProfileOperations(ProfileOperationsInterface):
    """ProfileOperations.py: the score groups computed from the profile alone."""

    def __init__(self, debugFlag=False, engine: Engine | None = None):
        super().__init__(debugFlag)
        self._engine = engine

    @property
    def engine(self) -> Engine:
        return self._engine or get_engine()

    # ---- batched forms: (n, k) scores and (n,) status bits ------------------------------
    def getSinusoidFittings_batch(self, profiles):
        p = _u8_rows(profiles)
        return self.engine.sinusoid4(p, np.zeros((len(p), PFE_NSCAL)))

    def getGaussianFittings_batch(self, profiles):
        p = _u8_rows(profiles)
        return self.engine.gauss7(p, np.zeros((len(p), PFE_NSCAL)))

    # ---- per candidate (the reference's signatures) --------------------------------------
    def getSinusoidFittings(self, profile):
        """:190-376 -> [chi^2 sine / maxima, chi^2 sine^2 / maxima, len(diff), sum residuals]"""
        out, st = self.getSinusoidFittings_batch(profile)
        _raise_failed(st)
        return [float(v) for v in out[0]]

    def getGaussianFittings(self, profile):
        """:595-770 -> scores 5-11."""
        out, st = self.getGaussianFittings_batch(profile)
        _raise_failed(st)
        return [float(v) for v in out[0]]

    # ---- the per-fit methods ---------------------------------------------------------------
    # The reference calls each of these only from inside its group method (getSinusoidFittings
    # :370-371; getGaussianFittings :640-760; fitDoubleGaussian :1330-1420 calls
    # fitDoubleGaussianWithBackground), and the engine runs each fit only as a stage of its
    # group's pooled kernel chain (csrc/bates_sine_dm_sub.hip k_sineg; csrc/bates_gauss.h
    # k_ghistg / k_gfixg / k_gt1g / k_gdgg / k_gdg8g), whose intermediate parameters, fit
    # arrays and FWHMs never leave the device.  So none is a group of its own: each raises,
    # naming the group method (and its columns) that carries the fit's result.
    def _per_fit(self, name, ref, group, cols):
        raise NotImplementedError(
            f"ProfileOperations.{name} ({ref}) is not a score group of its own: the fit runs "
            f"inside {group} (include/pfe.h), whose result is {cols}; call {group} on the "
            f"profile instead")

    def fitSine(self, yData, maxima):
        """ProfileOperations.py:380-491 (chi^2 of the fixed-amplitude sine fit).  Runs inside
        getSinusoidFittings / pfe_sinusoid4: s1 = fitSine(profile, maxima) / maxima with the
        profile's own maxima (:370)."""
        self._per_fit("fitSine", "ProfileOperations.py:380-491", "getSinusoidFittings",
                      "s1 = fitSine(profile, maxima) / maxima")

    def fitSineSqr(self, yData, maxima):
        """:495-587 (chi^2 of the sine^2 fit, its residual sign kept).  Runs inside
        getSinusoidFittings / pfe_sinusoid4: s2 = fitSineSqr(profile, maxima) / maxima (:371)."""
        self._per_fit("fitSineSqr", "ProfileOperations.py:495-587", "getSinusoidFittings",
                      "s2 = fitSineSqr(profile, maxima) / maxima")

    def fitGaussian(self, xData, yData):
        """:774-983 (Gaussian fit to a Freedman-Diaconis histogram: of the profile's
        derivative and of the profile, :660, :681).  Runs inside getGaussianFittings /
        pfe_gauss7 (k_ghistg): s5-s7 (:720-722)."""
        self._per_fit("fitGaussian", "ProfileOperations.py:774-983", "getGaussianFittings",
                      "s5-s7 (columns 0-2 of pfe_gauss7)")

    def fitGaussianFixedWidthBins(self, xData, yData, bins):
        """:988-1057 (the fixed-centre fit to the profile histogram, :701).  Runs inside
        getGaussianFittings / pfe_gauss7 (k_gfixg): s5, s6."""
        self._per_fit("fitGaussianFixedWidthBins", "ProfileOperations.py:988-1057",
                      "getGaussianFittings", "s5-s6 (columns 0-1 of pfe_gauss7)")

    def fitGaussianWithBackground(self, xData, yData):
        """:1194-1264 (Gaussian plus background).  Runs inside getGaussianFittings /
        pfe_gauss7 (k_gt1g, called by fitGaussianT1 :1123): s8, s9."""
        self._per_fit("fitGaussianWithBackground", "ProfileOperations.py:1194-1264",
                      "getGaussianFittings", "s8-s9 (columns 3-4 of pfe_gauss7)")

    def fitGaussianT1(self, yData):
        """:1061-1132 (the T1 fit).  Runs inside getGaussianFittings / pfe_gauss7 (k_gt1g):
        s8, s9."""
        self._per_fit("fitGaussianT1", "ProfileOperations.py:1061-1132", "getGaussianFittings",
                      "s8-s9 (columns 3-4 of pfe_gauss7)")

    def fitDoubleGaussianT2(self, yData):
        """:1136-1190 (the T2 double-Gaussian test).  Runs inside getGaussianFittings /
        pfe_gauss7 (k_gdgg peel passes + k_gdg8g): s10, s11."""
        self._per_fit("fitDoubleGaussianT2", "ProfileOperations.py:1136-1190",
                      "getGaussianFittings", "s10-s11 (columns 5-6 of pfe_gauss7)")

    def fitDoubleGaussian(self, yData):
        """:1268-1428 (peel passes, then the 8-parameter fit and the combination rule; called
        by fitDoubleGaussianT2 :1183).  Runs inside getGaussianFittings / pfe_gauss7 (k_gdgg +
        k_gdg8g): s10, s11."""
        self._per_fit("fitDoubleGaussian", "ProfileOperations.py:1268-1428",
                      "getGaussianFittings", "s10-s11 (columns 5-6 of pfe_gauss7)")

    def fitDoubleGaussianWithBackground(self, yData, p0):
        """:1432-1483 (the 8-parameter fit from fitDoubleGaussian's start point, :1411).  Runs inside
        getGaussianFittings / pfe_gauss7 (k_gdg8g): s10, s11."""
        self._per_fit("fitDoubleGaussianWithBackground", "ProfileOperations.py:1432-1483",
                      "getGaussianFittings", "s10-s11 (columns 5-6 of pfe_gauss7)")


class PHCXOperations(ProfileOperations):
    """PHCXOperations.py: the groups read from the candidate file itself.  `data` is what the
    reference passes -- its minidom Document (PHCXFile.rawdata) or that XML's text, read at
    `section` -- or a parsed candidate (phcx.parse) or a candidate path, whose `section` is
    checked against the file type (1 PHCX, 0 SUPERB)."""

    @staticmethod
    def _cand(data, section=None):
        if isinstance(data, str):
            c = _phcx.parse(data)
        elif hasattr(data, "toxml") or isinstance(data, (bytes, bytearray)):
            # the reference's own xmldata (minidom Document, PHCXFile.py:103-104) or its text
            c = _phcx.parse_document(data, 1 if section is None else section)
        else:
            c = data
        if section is not None and int(section) != c.section:
            raise ValueError(f"section {section}: this candidate is read from section {c.section}")
        return c

    def getCandidateParameters_batch(self, scal):
        return self.engine.params4(np.asarray(scal, dtype=np.float64))

    def getDMFittings_batch(self, dmcurves, scal):
        return self.engine.dmfit4(np.asarray(dmcurves, dtype=np.float64),
                                  np.asarray(scal, dtype=np.float64))

    def getSubbandParameters_batch(self, profiles, subbands, scal):
        """Byte-valued profiles and sub-bands (the rule of _profile_rows) go to pfe_subband3;
        anything else (normalised or baseline-subtracted data) to pfe_subband3_f64 -- or, when
        the profile and the sub-bands are both float32, to pfe_subband3_f32 as they are, with
        nothing widened on the host (the same values: pfe.h)."""
        scal = np.asarray(scal, dtype=np.float64)
        sub = np.asarray(subbands)
        sf = sub.dtype != np.uint8 and bool(sub.size) and (
            sub.min() < 0 or sub.max() > 255 or not np.array_equal(sub, np.round(sub)))
        if isinstance(profiles, np.ndarray) and profiles.dtype == np.float32 and sub.dtype == np.float32:
            p32 = profiles[None, :] if profiles.ndim == 1 else profiles
            if sf or (p32.size and (p32.min() < 0 or p32.max() > 255 or
                                    not np.array_equal(p32, np.round(p32)))):
                return self.engine.subband3_f32(np.ascontiguousarray(p32), np.ascontiguousarray(sub),
                                                scal)
        prof, pf = _profile_rows(profiles)
        if pf or sf:
            return self.engine.subband3_f64(np.ascontiguousarray(prof, dtype=np.float64),
                                            np.ascontiguousarray(sub, dtype=np.float64), scal)
        return self.engine.subband3(prof, sub.astype(np.uint8, copy=False), scal)

    def getCandidateParameters(self, data, section=None):
        """:81-112 -> [period (ms), snr, dm, width] as the method returns them (PHCXFile
        applies filterScore(13/14) when it stores s13/s14)."""
        c = self._cand(data, section)
        out, _st = self.getCandidateParameters_batch(c.scal[None, :])
        return [float(v) for v in out[0]]

    def getDMFittings(self, data, section=None):
        """:121-233 -> [peak, |1 - Prop|, Shift, chi_theo] (s18 = filterScore(18, Shift))."""
        c = self._cand(data, section)
        if len(c.dm_curve) < 3:  # leastsq with fewer rows than parameters raises
            raise Exception(status_error(0x004))
        out, st = self.getDMFittings_batch(c.dm_curve[None, :], c.scal[None, :])
        _raise_failed(st)
        return tuple(float(v) for v in out[0])  # the reference returns a tuple (:233)

    def getSubbandParameters(self, section=None, data=None, profile=None):
        """:305-349 -> [RMS of peak positions, mean pair correlation, correlation integral]
        ([0.0, 0.0, 0.0] without data and profile, :331-332)."""
        if data is None and profile is None:
            return [0.0, 0.0, 0.0]
        c = self._cand(data, section)
        prof = c.profile if profile is None else profile
        out, st = self.getSubbandParameters_batch(prof, c.subbands[None], c.scal[None, :])
        _raise_failed(st)
        return [float(v) for v in out[0]]


def _profile_rows(profile):
    """Rows of a profile argument and whether they take the float path: byte-valued profiles
    stay uint8 (the kernels PHCX files use), anything else goes as float64."""
    try:
        return _u8_rows(profile), False
    except TypeError:
        p = np.asarray(profile, dtype=np.float64)
        return np.ascontiguousarray(p[None, :] if p.ndim == 1 else p), True


class PFDOperations(ProfileOperations):
    """PFDOperations.py:62-466: the groups of a PRESTO fold.  `data` is what the reference
    passes -- the PFDFile object (candidate.PFDFile, or any object with the fold's attributes
    as PFDFile.load sets them) -- or a fold read by pfd.read, or a .pfd path."""

    @staticmethod
    def _fold(data):
        if isinstance(data, str):
            return _pfd.read(data)
        inner = getattr(data, "data", None)
        return inner if isinstance(inner, _pfd.PFDData) else data

    def _inputs(self, data):
        return _pfd.batch_inputs([self._fold(data)])

    def _kill(self, data):
        """Keywords of the PFD calls for a fold with killed intervals or sub-bands
        (PFDFile.kill_intervals / kill_subbands): its masks, and the average derived from the
        zapped cube on the device.  {} for a fold with nothing killed -- unless it carries no
        average (avgprof None: read with avgprof=False), which the device then derives."""
        fold = self._fold(data)
        parts, subs = _pfd.kill_masks([fold])
        if parts is None:
            return {"derive_avgprof": True} if getattr(fold, "avgprof", 0.0) is None else {}
        return dict(kill_parts=parts, kill_subs=subs, derive_avgprof=True)

    # ---- batched forms -------------------------------------------------------------------
    def getSinusoidFittings_batch(self, profiles):
        p, f64 = _profile_rows(profiles)
        return self.engine.sinusoid4_f64(p) if f64 else super().getSinusoidFittings_batch(p)

    def getGaussianFittings_batch(self, profiles):
        p, f64 = _profile_rows(profiles)
        return self.engine.gauss7_f64(p) if f64 else super().getGaussianFittings_batch(p)

    def getCandidateParameters_batch(self, profs, subfreqs, scal, **kill):
        """Folds of one shape, as pfd.batch_inputs packs them -> ((n, 4), status).  kill (this
        and the next two): kill_parts / kill_subs / derive_avgprof as Engine.pfd_params4 takes."""
        return self.engine.pfd_params4(profs, subfreqs, scal, **kill)

    def getDMFittings_batch(self, profs, subfreqs, scal, **kill):
        return self.engine.pfd_dmfit4(profs, subfreqs, scal, **kill)

    def getSubbandParameters_batch(self, profs, subfreqs, scal, **kill):
        return self.engine.pfd_subband3(profs, subfreqs, scal, **kill)

    # ---- per fold (the reference's signatures) -------------------------------------------
    def getCandidateParameters(self, data):
        """:93-233 -> [period (ms), snr, dm, width] as the method returns them (PFDFile applies
        filterScore(13/14) when it stores s13/s14)."""
        out, _st = self.getCandidateParameters_batch(*self._inputs(data), **self._kill(data))
        return [float(v) for v in out[0]]

    def _dm_curve(self, data):
        r = self.engine.pfd_dmprof(*self._inputs(data), profile=False, lyon8=False, **self._kill(data))
        if int(r["status"][0]) & PFE_ST_PFD_DMCURVE_FAIL:  # numdms == 1: dms[0] raises
            raise Exception("DM curve extraction exception")
        return r["chis"][0]

    def getDMCurveData(self, data):
        """:242-252 -- the float32 chi^2-vs-DM curve over span(dms[0], dms[-1], 100)."""
        return self._dm_curve(data)

    def getDMCurveDataNormalised(self, data):
        """:254-272 -- 255./max(y)*y of that curve, in float32 as numpy evaluates it."""
        y = self._dm_curve(data)
        return np.float32(255.0) / max(y) * y

    def getDMFittings(self, data):
        """:274-393 -> (peak, |1 - Prop|, Shift, chi_theo) (s18 = filterScore(18, Shift))."""
        out, st = self.getDMFittings_batch(*self._inputs(data), **self._kill(data))
        _raise_failed(st)
        return tuple(float(v) for v in out[0])

    def getSubbandParameters(self, data=None, profile=None):
        """:401-441 -> [RMS of peak positions, mean pair correlation, correlation integral];
        [0.0, 0.0, 0.0] with neither argument (:425-426).

        The boxcar width is the fold's own: the reference reads ``self.width``, which an
        earlier getCandidateParameters call on the same fold left behind, and the kernel
        derives the same width from the fold.  ``profile`` is accepted only when it is None
        or equals the fold's own 0..255 profile (what PFDFile passes); the kernel correlates
        the sub-bands with that profile, so any other raises ValueError."""
        if data is None and profile is None:
            return [0.0, 0.0, 0.0]
        if data is None:
            raise ValueError("getSubbandParameters: a profile without its fold")
        ins = self._inputs(data)
        if profile is not None:
            own = self.engine.pfd_dmprof(*ins, chis=False, lyon8=False, **self._kill(data))["profile"][0]
            given = np.asarray(profile, dtype=np.float64)
            if given.shape != own.shape or not np.array_equal(given, own, equal_nan=True):
                raise ValueError("getSubbandParameters: only the fold's own profile "
                                 "(PFDFile.getProfile()) is supported")
        out, st = self.getSubbandParameters_batch(*ins, **self._kill(data))
        _raise_failed(st)
        return [float(v) for v in out[0]]
