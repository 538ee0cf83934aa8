"""Dihedral angles and buffered rotamer states (reference
enspara/geometry/rotamer.py) on the device (csrc/ek_rotamer.hip).

``_rotamers`` is a state machine along time; the device runs it as a scan of
composed basin -> basin maps, chunk by chunk, all dihedrals of a trajectory in
one call, and computes the dihedral angles from the coordinates in the same
pass when asked to.

Where this differs from the reference, on purpose:

* There is no mdtraj here, so nothing derives atom indices from a topology:
  ``dihedral_angles`` and the ``*_rotamers`` functions take coordinates
  (``[frames, atoms, 3]``, or any object with an ``.xyz`` attribute) and the
  ``[n, 4]`` atom indices of the dihedrals.
* Angles are float32 (mdtraj's are) and are compared in float64 after the exact
  widening, against float64 gates; an array of another type is converted to
  float32 first.
* Angles are checked: finite and in ``[0, 360)``, else ``DataInvalid``.  The
  reference leaves the state -1 (frame 0) or writes state ``n_basins`` (later
  frames) for an angle of 360.
* A *shifted* angle that rounds to exactly 360.0 in float32 counts as the last
  basin (same two reference behaviours).
* At most 8 basins (``MAX_BASINS``), boundaries strictly increasing from 0 to
  360, ``0 <= buffer_width < 360 / n_basins``: else ``DataInvalid``.
"""
import numpy as np

from .. import _lib, exception

__all__ = ["dihedral_angles", "rotamers", "_rotamers", "rotamer_states",
           "dihedral_rotamers", "get_gates", "is_buffered_transition", "phi_rotamers",
           "psi_rotamers", "chi_rotamers", "all_rotamers", "MAX_BASINS", "KINDS", "SCAN_CHUNK"]

MAX_BASINS = 8
# frames of one call
MAX_FRAMES = 2 ** 27
# frames of one chunk of the state scan (ROT_CHUNK of csrc/ek_rotamer.hip)
SCAN_CHUNK = 256
# the reference's boundaries and shifts (phi_rotamers, psi_rotamers, chi_rotamers)
KINDS = {"phi": ([0, 180, 360], 0), "psi": ([0, 160, 360], 100),
         "chi": ([0, 120, 240, 360], 0)}


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)


# ---- the reference's host one-liners ---------------------------------------------
def get_gates(cur_state, hard_boundaries, buffer_width):
    """The gates a dihedral in basin ``cur_state`` must leave through for a
    buffered transition: the basin's lower boundary (0 read as 360) minus the
    buffer, its upper boundary (360 read as 0) plus the buffer."""
    s = int(cur_state)
    lower, upper = hard_boundaries[s], hard_boundaries[s + 1]
    lower = 360 if lower == 0 else lower
    upper = 0 if upper == 360 else upper
    return lower - buffer_width, upper + buffer_width


def is_buffered_transition(cur_state, new_angle, hard_boundaries, buffer_width):
    """Whether ``new_angle`` has left the gates of basin ``cur_state`` (both
    ends closed; the wrap-around form where the upper gate lies below the
    lower one; equal gates never transition)."""
    lower, upper = get_gates(cur_state, hard_boundaries, buffer_width)
    if upper < lower:
        return bool(upper <= new_angle <= lower)
    if upper > lower:
        return not (lower <= new_angle <= upper)
    return False


# ---- validation (before any device call) -----------------------------------------------
def _boundaries(hard_boundaries, buffer_width):
    hb = np.asarray(hard_boundaries, dtype=np.float64)
    if hb.ndim != 1 or len(hb) < 2:
        raise exception.DataInvalid(
            "hard_boundaries is a list of at least two numbers, got %r" % (hard_boundaries,))
    n_basins = len(hb) - 1
    if n_basins > MAX_BASINS:
        raise exception.DataInvalid(
            "%d basins: the device assigns at most %d" % (n_basins, MAX_BASINS))
    if hb[0] != 0 or hb[-1] != 360:
        raise exception.DataInvalid('hard_boundaries list must start with 0 and '
                                    'end with 360, list was %s.' % (hard_boundaries,))
    if not np.all(np.diff(hb) > 0):
        raise exception.DataInvalid(
            "hard_boundaries must increase, list was %s." % (hard_boundaries,))
    w = float(buffer_width)
    if not (w >= 0 and w < 360. / n_basins):
        raise exception.DataInvalid('Buffer width (got %s) must be between 0 and '
                                    '360 / %d degrees.' % (buffer_width, n_basins))
    return hb


def _angles(angles):
    a = np.asarray(angles)
    if a.ndim != 2 or a.shape[1] < 1:
        raise exception.DataInvalid(
            "angles are [frames] or [frames, dihedrals], not %s" % (a.shape,))
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size and not (np.all(np.isfinite(a)) and a.min() >= 0 and a.max() < 360):
        raise exception.DataInvalid("angles must be finite and lie in [0, 360) degrees")
    if len(a) > MAX_FRAMES:
        raise exception.DataInvalid("No support for more than %d frames a call." % MAX_FRAMES)
    return a


def _xyz(xyz):
    x = np.asarray(getattr(xyz, "xyz", xyz))
    if x.ndim != 3 or x.shape[2] != 3 or x.shape[1] < 1:
        raise exception.DataInvalid(
            "coordinates are [frames, atoms, 3], not %s" % (x.shape,))
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not np.all(np.isfinite(x)):
        raise exception.DataInvalid("coordinates must be finite")
    if len(x) > MAX_FRAMES:
        raise exception.DataInvalid("No support for more than %d frames a call." % MAX_FRAMES)
    return x


def _quads(atom_indices, n_atoms):
    q = np.asarray(atom_indices)
    if q.ndim != 2 or q.shape[1] != 4 or len(q) < 1 or not np.issubdtype(q.dtype, np.integer):
        raise exception.DataInvalid(
            "atom indices are [n, 4] integers, got %s of %s" % (q.shape, q.dtype))
    if q.min() < 0 or q.max() >= n_atoms:
        raise exception.DataInvalid(
            "atom indices must lie in [0, %d); found %d .. %d" % (n_atoms, q.min(), q.max()))
    return np.ascontiguousarray(q, dtype=np.int32)


def _tables(kind, n, boundaries, shifts, buffer_width):
    """-> (kind uint8 [n], n_basins int32 [k], hb float64 [k, 9], shift float32 [k])"""
    if len(boundaries) != len(shifts) or not 1 <= len(boundaries) <= 255:
        raise exception.DataInvalid("one shift per set of boundaries, 1 to 255 kinds")
    kind = np.asarray(kind)
    if kind.shape != (n,) or not np.issubdtype(kind.dtype, np.integer):
        raise exception.DataInvalid("one integer kind per dihedral (%d), got %s" % (n, kind.shape,))
    if kind.min() < 0 or kind.max() >= len(boundaries):
        raise exception.DataInvalid("kinds must lie in [0, %d)" % len(boundaries))
    hb = np.zeros((len(boundaries), MAX_BASINS + 1))
    nb = np.zeros(len(boundaries), dtype=np.int32)
    for k, b in enumerate(boundaries):
        b = _boundaries(b, buffer_width)
        nb[k] = len(b) - 1
        hb[k, :len(b)] = b
    shift = np.asarray(shifts, dtype=np.float32)
    if not np.all(np.isfinite(shift)):
        raise exception.DataInvalid("shifts must be finite")
    return np.ascontiguousarray(kind, dtype=np.uint8), nb, hb, shift


# ---- device calls --------------------------------------------------------------------------
def dihedral_angles(xyz, atom_indices, device=0):
    """Dihedral angles in degrees, ``[frames, n]`` float32 in ``[0, 359.5]``:
    mdtraj's ``atan2((b1 . c1) |b2|, c1 . c2)`` in float32 and the reference's
    transforms (``< 0 -> + 360``, ``> 359.5 -> 359.5``)."""
    x = _xyz(xyz)
    q = _quads(atom_indices, x.shape[1])
    out = np.zeros((len(x), len(q)), dtype=np.float32)
    _check(_lib.load().ek_dihedral_angles(int(device), _lib.f32p(x), len(x), x.shape[1],
                                          _lib.i32p(q), len(q), _lib.f32p(out), None))
    return out


def rotamer_states(angles, kind, boundaries, shifts, buffer_width=15, device=0,
                   timing=None):
    """Rotamer states of ``angles`` ([frames, n] degrees), dihedral ``j`` being of
    kind ``kind[j]`` with the boundaries ``boundaries[kind[j]]`` and the shift
    ``shifts[kind[j]]`` (subtracted in float32, 360 added where the result is
    negative).  -> uint8 ``[frames, n]``.  ``timing``: an array of two that
    receives the milliseconds of the device's kernels."""
    a = _angles(angles)
    k, nb, hb, sh = _tables(kind, a.shape[1], boundaries, shifts, buffer_width)
    out = np.zeros(a.shape, dtype=np.uint8)
    _check(_lib.load().ek_rotamer_states(
        int(device), _lib.f32p(a), len(a), a.shape[1], _lib.u8p(k), len(nb), _lib.i32p(nb),
        _lib.f64p(hb), _lib.f32p(sh), float(buffer_width), _lib.u8p(out),
        None if timing is None else _lib.f64p(timing)))
    return out


def dihedral_rotamers(xyz, atom_indices, kind, boundaries, shifts, buffer_width=15,
                      return_angles=False, device=0, timing=None):
    """``rotamer_states(dihedral_angles(xyz, atom_indices), ...)`` in one pass
    over the coordinates, without storing the angles (unless asked for): the
    same states bit for bit.  -> states, or (states, angles)."""
    x = _xyz(xyz)
    q = _quads(atom_indices, x.shape[1])
    k, nb, hb, sh = _tables(kind, len(q), boundaries, shifts, buffer_width)
    out = np.zeros((len(x), len(q)), dtype=np.uint8)
    ang = np.zeros((len(x), len(q)), dtype=np.float32) if return_angles else None
    _check(_lib.load().ek_dihedral_rotamers(
        int(device), _lib.f32p(x), len(x), x.shape[1], _lib.i32p(q), len(q), _lib.u8p(k),
        len(nb), _lib.i32p(nb), _lib.f64p(hb), _lib.f32p(sh), float(buffer_width),
        _lib.u8p(out), None if ang is None else _lib.f32p(ang),
        None if timing is None else _lib.f64p(timing)))
    return (out, ang) if return_angles else out


def rotamers(angles, hard_boundaries, buffer_width=15, shift=0, device=0):
    """Rotamer state assignment for a trajectory of dihedral angles using a
    buffered transition approach (the reference's ``_rotamers``).

    Parameters
    ----------
    angles : array-like, shape=(n_frames,) or (n_frames, n_dihedrals)
        Dihedral angles in degrees within [0, 360).
    hard_boundaries : array-like, shape=(n_basins + 1,)
        The boundaries of the rotamer basins, from 0 to 360.
    buffer_width : number, default=15
        The buffer on either side of a boundary; 0 is no buffer.
    shift : number, default=0
        Subtracted from the angles first (in float32; 360 is added where the
        result is negative), as ``psi_rotamers`` does with 100.

    Returns
    -------
    rotamers : int16 array of the shape of ``angles``
    """
    a = np.asarray(angles)
    one = a.ndim == 1
    if one:
        a = a[:, None]
    if a.ndim != 2:
        raise exception.DataInvalid(
            "angles are [frames] or [frames, dihedrals], not %s" % (a.shape,))
    _boundaries(hard_boundaries, buffer_width)
    if len(a) == 0:
        return np.zeros(np.asarray(angles).shape, dtype=np.int16)
    out = rotamer_states(a, np.zeros(a.shape[1], dtype=np.int64), [hard_boundaries], [shift],
                         buffer_width, device).astype(np.int16)
    return out[:, 0] if one else out


_rotamers = rotamers


def _one_kind(name, xyz, atom_indices, buffer_width, device):
    hb, shift = KINDS[name]
    q = np.asarray(atom_indices)
    states = dihedral_rotamers(xyz, q, np.zeros(len(q), dtype=np.int64), [hb], [shift],
                               buffer_width, device=device)
    return (states.astype(np.int16), q,
            (len(hb) - 1) * np.ones(len(q), dtype=np.int16))


def phi_rotamers(xyz, atom_indices, buffer_width=15, device=0):
    """-> (rotamers int16 [frames, n], atom_indices, n_states): boundaries
    [0, 180, 360]."""
    return _one_kind("phi", xyz, atom_indices, buffer_width, device)


def psi_rotamers(xyz, atom_indices, buffer_width=15, device=0):
    """As ``phi_rotamers``: angles shifted by 100, boundaries [0, 160, 360]."""
    return _one_kind("psi", xyz, atom_indices, buffer_width, device)


def chi_rotamers(xyz, atom_indices, buffer_width=15, device=0):
    """As ``phi_rotamers``: boundaries [0, 120, 240, 360], three states."""
    return _one_kind("chi", xyz, atom_indices, buffer_width, device)


def check_dihedrals(dihedrals):
    """``dihedrals`` as the mapping {"phi": [n, 4], "psi": ..., "chi": ...} (any
    of the three) -> (atom indices [n, 4] in the order phi, psi, chi, kind [n],
    n_states [n] int16)."""
    if dihedrals is None:
        raise exception.DataInvalid(
            "`dihedrals` is required: a mapping {'phi': [n, 4], 'psi': ..., 'chi': ...} of "
            "atom indices (there is no mdtraj here to derive them from a topology).")
    if not hasattr(dihedrals, "keys") or not set(dihedrals.keys()) <= set(KINDS) or \
            not len(dihedrals):
        raise exception.DataInvalid(
            "`dihedrals` maps some of 'phi', 'psi', 'chi' to [n, 4] atom indices, got %r"
            % (dihedrals,))
    quads, kind, n_states = [], [], []
    for k, name in enumerate(("phi", "psi", "chi")):
        if name not in dihedrals:
            continue
        q = np.asarray(dihedrals[name])
        if q.ndim != 2 or q.shape[1] != 4 or not np.issubdtype(q.dtype, np.integer):
            raise exception.DataInvalid(
                "dihedrals[%r] holds [n, 4] integer atom indices, got %s" % (name, q.shape,))
        quads.append(q)
        kind.append(np.full(len(q), k))
        n_states.append(np.full(len(q), len(KINDS[name][0]) - 1, dtype=np.int16))
    quads = np.concatenate(quads, axis=0)
    if len(quads) == 0:
        raise exception.DataInvalid("`dihedrals` holds no dihedral")
    return quads, np.concatenate(kind), np.concatenate(n_states)


def all_rotamers(xyz, dihedrals, buffer_width=15, device=0):
    """Compute the rotameric states of a trajectory over time.

    Parameters
    ----------
    xyz : array [frames, atoms, 3], or an object with such an ``.xyz``
    dihedrals : mapping {"phi": [n, 4], "psi": [n, 4], "chi": [n, 4]}
        The atom indices of the dihedrals of each kind (any of the three).
    buffer_width : number, default=15

    Returns
    -------
    all_rotamers : int16 [frames, n_dihedrals], columns in the order phi, psi, chi
    all_atom_inds : [n_dihedrals, 4]
    all_n_states : int16 [n_dihedrals]: 2 for phi and psi, 3 for chi
    """
    quads, kind, n_states = check_dihedrals(dihedrals)
    names = ("phi", "psi", "chi")
    states = dihedral_rotamers(xyz, quads, kind, [KINDS[k][0] for k in names],
                               [KINDS[k][1] for k in names], buffer_width, device=device)
    return states.astype(np.int16), quads, n_states
