"""PRESTO .pfd candidate files: host-side reader and synthetic writer.

Reader semantics follow PFDFile.load (PulsarFeatureExtractor/src/PFDFile.py:96-252):
  * byte order: little-endian unless one of the first five int32 exceeds 100000 in
    magnitude, then big-endian (:113-118)
  * header ints, four length-prefixed strings, an optional 16+16-byte RA/Dec block (present
    when the next 16 bytes are all in '0123456789:.-\\0', :126-141), doubles/floats of the
    fold, dms / periods / pdots, profs[npart][nsub][proflen] and foldstats[npart][nsub][7]
  * derived quantities: binspersec = fold_p1 * proflen, chanpersub = numchan // nsub (Py2
    integer '/'), subfreqs, avgprof = (profs / proflen).sum(), varprof = sum of the
    prof_var foldstats (:219-252, calc_varprof :314-327)
A truncated profs/foldstats block leaves zeros, as the reference's per-row try/except does.
"""
from __future__ import annotations

import struct

import numpy as np

_POSN_CHARS = set(b"0123456789:.-\0")


class PFDData:
    """Header fields and arrays of one .pfd file (the attributes PFDFile.load sets)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def read(path: str, avgprof: bool = True) -> PFDData:
    """One .pfd file.  avgprof False: the pass over the cube for (profs / proflen).sum() is
    left out and the attribute is None (the PFD calls derive it on the device:
    Engine.pfd_dmprof(..., derive_avgprof=True))."""
    with open(path, "rb") as f:
        data = f.read()
    pos = 0

    def take(n):
        nonlocal pos
        if pos + n > len(data):
            raise struct.error("unpack requires a buffer of %d bytes" % n)
        b = data[pos:pos + n]
        pos += n
        return b

    head = take(20)
    sw = "<"
    if np.abs(np.asarray(struct.unpack("<5i", head), dtype=np.float64)).max() > 100000:
        sw = ">"
    numdms, numperiods, numpdots, nsub, npart = struct.unpack(sw + "5i", head)
    proflen, numchan, pstep, pdstep, dmstep, ndmfact, npfact = struct.unpack(sw + "7i", take(28))
    strs = []
    for _ in range(4):
        (ln,) = struct.unpack(sw + "i", take(4))
        strs.append(take(ln))
    test = take(16)
    if all(c in _POSN_CHARS for c in test):
        rastr = test[: test.find(b"\0")]
        test2 = take(16)
        decstr = test2[: test2.find(b"\0")]
        dt, start_t = struct.unpack(sw + "dd", take(16))
    else:
        rastr = decstr = b"Unknown"
        dt, start_t = struct.unpack(sw + "dd", test)
    end_t, tepoch, bepoch, avgvoverc, lofreq, chan_wid, bestdm = struct.unpack(sw + "7d", take(56))
    vals = {}
    for name in ("topo", "bary", "fold"):
        pw, _tmp = struct.unpack(sw + "2f", take(8))
        p1, p2, p3 = struct.unpack(sw + "3d", take(24))
        vals[name] = (pw, p1, p2, p3)
    orb = struct.unpack(sw + "7d", take(56))
    dms = np.asarray(struct.unpack(sw + "%dd" % numdms, take(8 * numdms)))
    periods = np.asarray(struct.unpack(sw + "%dd" % numperiods, take(8 * numperiods)))
    pdots = np.asarray(struct.unpack(sw + "%dd" % numpdots, take(8 * numpdots)))
    dt_ = np.dtype(np.float64).newbyteorder(sw)
    profs = np.zeros((npart, nsub, proflen), dtype=np.float64)
    nprof = npart * nsub * proflen
    avail = max(0, min(nprof, (len(data) - pos) // 8))
    if sw == "<":
        # row by row: a row that cannot be read completely stays zero (:170-176)
        rows = avail // proflen if proflen else 0
        flat = np.frombuffer(data, dtype=dt_, count=rows * proflen, offset=pos)
        profs.reshape(-1, proflen)[:rows] = flat.reshape(rows, proflen)
        pos += rows * proflen * 8
        if rows < npart * nsub:
            pos = len(data)
    else:
        if avail < nprof:
            raise struct.error("unpack requires a buffer of %d bytes" % (8 * nprof))
        profs[:] = np.frombuffer(data, dtype=dt_, count=nprof, offset=pos).reshape(profs.shape)
        pos += nprof * 8
    stats = np.zeros((npart, nsub, 7), dtype=np.float64)
    for ii in range(npart):
        for jj in range(nsub):
            if pos + 56 <= len(data):
                stats[ii, jj] = np.frombuffer(data, dtype=dt_, count=7, offset=pos)
                pos += 56
    binspersec = vals["fold"][1] * proflen
    chanpersub = numchan // nsub
    subdeltafreq = chan_wid * chanpersub
    losubfreq = lofreq + subdeltafreq - chan_wid
    subfreqs = np.arange(nsub, dtype="d") * subdeltafreq + losubfreq
    varprof = 0.0
    for part in range(npart):
        for sub in range(nsub):
            varprof += stats[part][sub][5]
    return PFDData(
        swap=sw, numdms=numdms, numperiods=numperiods, numpdots=numpdots, nsub=nsub,
        npart=npart, proflen=proflen, numchan=numchan, filenm=strs[0], candnm=strs[1],
        telescope=strs[2], pgdev=strs[3], rastr=rastr, decstr=decstr, dt=dt, startT=start_t,
        endT=end_t, tepoch=tepoch, bepoch=bepoch, avgvoverc=avgvoverc, lofreq=lofreq,
        chan_wid=chan_wid, bestdm=bestdm, topo_p1=vals["topo"][1], bary_p1=vals["bary"][1],
        fold_p1=vals["fold"][1], orb=orb, dms=dms, periods=periods, pdots=pdots, profs=profs,
        stats=stats, binspersec=binspersec, chanpersub=chanpersub, subdeltafreq=subdeltafreq,
        losubfreq=losubfreq, subfreqs=subfreqs, avgprof=(profs / proflen).sum() if avgprof else None,
        varprof=varprof, killed_subbands=[], killed_intervals=[])


def varprof(prof_var, kill_parts=None, kill_subs=None):
    """calc_varprof (PFDFile.py:314-326) for a batch: prof_var (..., npart, nsub), the
    foldstats' column 5 -> (...,) the sequential sum in (part, sub) order from 0.0, the rows of
    killed parts (..., npart) and sub-bands (..., nsub) skipped; a 1-D mask is for every fold.
    Skipping a term and adding +0.0 in its place give the same bits (x + 0.0 == x, and the sum
    starts from +0.0), so this is np.add.accumulate over np.where(kill, 0.0, v)."""
    v = np.asarray(prof_var, dtype=np.float64)
    if v.ndim < 2:
        raise ValueError("varprof: prof_var must be (..., npart, nsub)")
    kill = np.zeros(v.shape, dtype=bool)
    if kill_parts is not None:
        kill |= np.asarray(kill_parts).astype(bool)[..., :, None]
    if kill_subs is not None:
        kill |= np.asarray(kill_subs).astype(bool)[..., None, :]
    z = np.where(kill, 0.0, v).reshape(v.shape[:-2] + (-1,))
    if z.shape[-1] == 0:
        return np.zeros(v.shape[:-2])
    # accumulate is sequential (no pairwise blocks); 0.0 + z[0] is z[0] bit for bit but for
    # z[0] = -0.0, where the loop from 0.0 gives +0.0
    return np.add.accumulate(z, axis=-1)[..., -1] + 0.0


def parse_kill_list(text):
    """show_pfd's -killsubs / -killparts syntax: '0,3:5' -> [0, 3, 4, 5] (ranges inclusive)."""
    out = []
    for tok in str(text).split(","):
        tok = tok.strip()
        if not tok:
            continue
        lo, sep, hi = tok.partition(":")
        try:
            a = int(lo)
            b = int(hi) if sep else a
        except ValueError:
            raise ValueError(f"bad kill list {text!r}: {tok!r} is neither N nor LO:HI") from None
        if a < 0 or b < a:
            raise ValueError(f"bad kill list {text!r}: {tok!r} must be 0 <= LO <= HI")
        out.extend(range(a, b + 1))
    return out


def kill_masks(datas):
    """The killed_intervals / killed_subbands lists of PFDData of one shape as the uint8 masks
    of the PFD calls -> (kill_parts (n,npart), kill_subs (n,nsub)), or (None, None) when no
    fold has anything killed."""
    lists = [(getattr(d, "killed_intervals", None) or [], getattr(d, "killed_subbands", None) or [])
             for d in datas]
    if not any(kp or ks for kp, ks in lists):
        return None, None
    d0 = datas[0]
    parts = np.zeros((len(datas), d0.npart), dtype=np.uint8)
    subs = np.zeros((len(datas), d0.nsub), dtype=np.uint8)
    for i, (kp, ks) in enumerate(lists):
        parts[i, list(kp)] = 1
        subs[i, list(ks)] = 1
    return parts, subs


def delay_from_dm(dm, freq):
    """PFDOperations.delay_from_DM (:474-486): the dispersion delay in seconds at `freq` MHz,
    0.0 where the frequency is not positive."""
    freq = np.asarray(freq, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(freq > 0.0, dm / (0.000241 * freq * freq), 0.0)


def scrunch_plan(chanfreqs, dm, binspersec, nbin, fscr):
    """How Engine.pfd_scrunch makes sub-bands of fscr channels each, as prepfold does: the
    channels of a group aligned at `dm` on the group's centre, the groups left unaligned for
    the DM search.  chanfreqs (..., nchan) MHz, ascending or descending; dm and binspersec
    scalars or (...,) -> (rot int32 (..., nchan), subfreqs (..., G)), G = nchan / fscr:
      subfreqs[g] = 0.5 * (f[g*fscr] + f[g*fscr + fscr - 1])
      rot[c]      = int(floor((delay(dm, f[c]) - delay(dm, subfreqs[g])) * binspersec + 0.5))
    the left rotation of channel c in bins: positive below the centre (the pulse arrives later),
    negative above it.  The device reduces it mod nbin; a value beyond int32 is reduced here."""
    f = np.asarray(chanfreqs, dtype=np.float64)
    fscr = int(fscr)
    if f.ndim < 1 or fscr < 1 or f.shape[-1] % fscr:
        raise ValueError(f"scrunch_plan: fscr {fscr} does not divide nchan "
                         f"{f.shape[-1] if f.ndim else 0}")
    if int(nbin) < 1:
        raise ValueError(f"scrunch_plan: nbin {nbin}")
    groups = f.reshape(f.shape[:-1] + (f.shape[-1] // fscr, fscr))
    subfreqs = 0.5 * (groups[..., 0] + groups[..., -1])
    dm = np.asarray(dm, dtype=np.float64)[..., None]
    bps = np.asarray(binspersec, dtype=np.float64)[..., None]
    lag = delay_from_dm(dm, f) - np.repeat(delay_from_dm(dm, subfreqs), fscr, axis=-1)
    rot = np.floor(lag * bps + 0.5)
    if not np.isfinite(rot).all():
        raise ValueError("scrunch_plan: a rotation is not finite")
    if rot.size and np.abs(rot).max() >= 2.0 ** 31:
        rot = rot % float(nbin)
    return rot.astype(np.int32), subfreqs


def scrunch_route(nbin, bscr):
    """The route the scrunch kernels take for rows of nbin bins summed bscr at a time
    (csrc/launch.h pfd_scrunch_lds): 'lds' when a row, rounded up to a multiple of 4 values, and
    its nbin / bscr running sums fit 8192 doubles of LDS, else 'direct' (one lane per output
    bin).  The handle option pfd_scrunch_direct sends every shape the direct way; the bits are
    the same on both."""
    return "lds" if (int(nbin) + 3) // 4 * 4 + int(nbin) // int(bscr) <= 8192 else "direct"


def scrunch_scal(scal, bscr):
    """The scalars (..., 8) of a fold after Engine.pfd_scrunch summed bscr bins into one:
    binspersec / bscr; varprof * bscr (a bin of the summed profile is the sum of bscr bins, so
    its variance is bscr times a bin's); avgprof NaN, to be derived from the scrunched fold
    (derive_avgprof=True).  The rest unchanged."""
    bscr = int(bscr)
    if bscr < 1:
        raise ValueError(f"scrunch_scal: bscr {bscr}")
    out = np.array(scal, dtype=np.float64)
    out[..., 1] = out[..., 1] / bscr
    out[..., 2] = np.nan
    out[..., 3] = out[..., 3] * bscr
    return out


def write(path: str, *, profs, stats=None, dms, bestdm, fold_p1, bary_p1=None, lofreq=1200.0,
          chan_wid=1.0, numchan=None, dt=6.4e-5, big_endian=False, with_posn=True,
          periods=None, pdots=None):
    """Synthetic .pfd with the PRESTO layout PFDFile.load reads."""
    profs = np.asarray(profs, dtype=np.float64)
    npart, nsub, proflen = profs.shape
    if numchan is None:
        numchan = nsub * 4
    if stats is None:
        stats = np.zeros((npart, nsub, 7))
        stats[:, :, 0] = 1000.0
        stats[:, :, 5] = profs.var(axis=2) * proflen
    if bary_p1 is None:
        bary_p1 = fold_p1
    dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
    periods = np.asarray([fold_p1] if periods is None else periods, dtype=np.float64)
    pdots = np.asarray([0.0] if pdots is None else pdots, dtype=np.float64)
    sw = ">" if big_endian else "<"
    out = [struct.pack(sw + "5i", len(dms), len(periods), len(pdots), nsub, npart),
           struct.pack(sw + "7i", proflen, numchan, 1, 1, 1, 1, 1)]
    for s in (b"synthetic.dat", b"PSR_SYN", b"Parkes", b"/null"):
        out.append(struct.pack(sw + "i", len(s)) + s)
    if with_posn:
        out.append(b"12:34:56.7890\0\0\0")
        out.append(b"-12:34:56.789\0\0\0")
    out.append(struct.pack(sw + "dd", dt, 0.0))
    out.append(struct.pack(sw + "7d", 1000.0, 56000.0, 56000.5, 0.0, lofreq, chan_wid, bestdm))
    for p1 in (fold_p1, bary_p1, fold_p1):
        out.append(struct.pack(sw + "2f", 1.0, 0.0) + struct.pack(sw + "3d", p1, 0.0, 0.0))
    out.append(struct.pack(sw + "7d", *([0.0] * 7)))
    out.append(struct.pack(sw + "%dd" % len(dms), *dms))
    out.append(struct.pack(sw + "%dd" % len(periods), *periods))
    out.append(struct.pack(sw + "%dd" % len(pdots), *pdots))
    out.append(profs.astype(np.dtype(np.float64).newbyteorder(sw)).tobytes())
    out.append(np.asarray(stats, dtype=np.float64).astype(np.dtype(np.float64).newbyteorder(sw)).tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(out))


def batch_inputs(datas):
    """Dense pfe_pfd_dmprof inputs for PFDData of one (npart, nsub, proflen) shape.  A fold
    read without its average (avgprof None) gets NaN in scal[:, 2]: score it with
    derive_avgprof=True."""
    n = len(datas)
    d0 = datas[0]
    profs = np.empty((n, d0.npart, d0.nsub, d0.proflen), dtype=np.float64)
    subfreqs = np.empty((n, d0.nsub), dtype=np.float64)
    scal = np.zeros((n, 8), dtype=np.float64)
    for i, d in enumerate(datas):
        profs[i] = d.profs
        subfreqs[i] = d.subfreqs
        dms = np.atleast_1d(d.dms)
        avg = np.nan if d.avgprof is None else d.avgprof
        scal[i] = (d.bestdm, d.binspersec, avg, d.varprof, dms[0], dms[-1], d.numdms, d.bary_p1)
    return profs, subfreqs, scal
