"""Stroke simplification in front of the loaders: Ramer-Douglas-Peucker on the device (skf_rdp_f32, skf_stroke3_simplify;
include/skf.h has the rule, DESIGN.md section 3p the reasons) and the host helpers that turn raw vector drawings into the
stroke-3 sketches the chunk files hold.  The device functions have no CPU fallback; the helpers are plain numpy.

Conventions.  A polyline is an (n, 2) array of absolute positions; a drawing is a list of polylines, one per stroke.  A stroke-3
sketch holds one row (dx, dy, pen) per point, the first row's offset counted from (0, 0), pen == 1 on the last row of a stroke.
"""
import numpy as np

from .preprocess import _device, pack_ragged

EXACT_POSITIONS = 1 << 23      # integer sketches: below this, positions and the offsets between any two of them are exact in fp32


def _integer_limits(sketches):
    """Per sketch: is its dtype an integer one, and the range of that dtype (0, 0 for the others)."""
    n = len(sketches)
    is_int, lo, hi = np.zeros(n, bool), np.zeros(n, np.float64), np.zeros(n, np.float64)
    for i, s in enumerate(sketches):
        dtype = np.asarray(s).dtype
        if np.issubdtype(dtype, np.integer):
            info = np.iinfo(dtype)
            is_int[i], lo[i], hi[i] = True, info.min, info.max
    return is_int, lo, hi


def _check_positions(flat, offsets, is_int):
    """Integer sketches stay integers only while the fp32 running sum is exact: refuse one whose position leaves +-2^23.  (Read
    from the packed float32 rows: an offset that the packing rounded is at least 2^24 and moves a position out of the range.)"""
    lens = np.diff(offsets)
    run = np.cumsum(flat[:, :2], axis=0, dtype=np.float64)
    start = np.concatenate([np.zeros((1, 2)), run])[offsets[:-1]]
    pos = run - np.repeat(start, lens, axis=0)
    bad = (np.abs(pos) >= EXACT_POSITIONS).any(axis=1) & np.repeat(is_int, lens)
    if bad.any():
        i = int(np.searchsorted(offsets, np.flatnonzero(bad)[0], side="right")) - 1
        raise ValueError("sketch %d: an integer sketch must stay within +-2^23 of its origin to be simplified exactly" % i)


def simplify_sketches(sketches, epsilon, device=None):
    """A list or object array of stroke-3 arrays -> the same, every stroke simplified at `epsilon` (in the units of the offsets).
    An integer dtype is preserved: on integer offsets the positions, and so the offsets between kept positions, are exact
    integers - as long as every position of the sketch, counted from (0, 0), lies within +-2^23, which is checked: ValueError
    otherwise, and ValueError too when an offset between kept rows (the sum of the dropped rows' offsets) does not fit the dtype.
    Any other dtype comes back as float32.  Stroke ends stay, so pen values and the stroke count do not change."""
    n = len(sketches)
    flat, offsets = pack_ragged(sketches)
    if len(flat) == 0:
        out = [np.array(np.asarray(s)[:, :3], copy=True) for s in sketches]
    else:
        is_int, lo, hi = _integer_limits(sketches)
        if is_int.any():
            _check_positions(flat, offsets, is_int)
        import torch
        from . import ops
        dev = _device(device)
        with torch.cuda.device(dev):
            out_flat, out_offsets = ops.stroke3_simplify(torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), epsilon)
            rows, offs = out_flat.cpu().numpy(), out_offsets.cpu().numpy()
        if is_int.any():
            kept = np.diff(offs)
            wide = ((rows[:, :2] < np.repeat(lo, kept)[:, None]) | (rows[:, :2] > np.repeat(hi, kept)[:, None])).any(axis=1)
            wide &= np.repeat(is_int, kept)
            if wide.any():
                i = int(np.searchsorted(offs, np.flatnonzero(wide)[0], side="right")) - 1
                raise ValueError("sketch %d: an offset between kept rows does not fit %s" % (i, np.asarray(sketches[i]).dtype.name))
        out = []
        for i, s in enumerate(sketches):
            dtype = np.asarray(s).dtype
            part = rows[offs[i]:offs[i + 1]]
            out.append(part.astype(dtype) if is_int[i] else part.copy())
    if isinstance(sketches, np.ndarray):
        arr = np.empty(n, dtype=object)
        for i, s in enumerate(out):
            arr[i] = s
        return arr
    return out


RESAMPLE_MAX_COORD = 16384     # SKF_RESAMPLE_MAX_COORD of include/skf.h: beyond it the arc length of a batch may overflow int64
RESAMPLE_ROW_BUDGET = 1 << 24  # resampled rows one device call may produce (128 MiB of points, 96 MiB of RDP state beside them)


def _pack_lines(lines):
    """-> (the polylines as (n, 2) arrays, offsets int64, xy float32 (P, 2))"""
    lines = [np.asarray(l).reshape(-1, 2) for l in lines]
    lens = np.fromiter((len(l) for l in lines), dtype=np.int64, count=len(lines))
    offsets = np.zeros(len(lines) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    parts = [l for l in lines if len(l)]
    xy = np.ascontiguousarray(np.concatenate(parts, axis=0), dtype=np.float32) if parts else np.zeros((0, 2), np.float32)
    return lines, offsets, xy


def _check_resample(xy, spacing, n_points):
    """The host-side refusals of the resampling helpers, before anything goes to the device."""
    if (spacing is None) == (n_points is None):
        raise ValueError("give exactly one of spacing and n_points")
    if spacing is not None:
        spacing = float(spacing)
        if not (spacing < 7e13 and spacing * 65536.0 > 0.5):     # (false for a NaN)
            raise ValueError("spacing must be finite, below 7e13, with rint(spacing * 2^16) >= 1 (got %r)" % spacing)
    else:
        n_points = int(n_points)
        if not 2 <= n_points <= 65536:
            raise ValueError("n_points must be in [2, 65536] (got %d)" % n_points)
    if len(xy) and not (np.abs(xy) <= RESAMPLE_MAX_COORD).all():     # (false for a NaN or an infinity too)
        raise ValueError("coordinates must be finite and within +-%d to be resampled (the arc length is summed in int64 units of "
                         "2^-16)" % RESAMPLE_MAX_COORD)
    return spacing, n_points


def _cut_by_rows(out_offsets, budget):
    """[(first, last + 1)] runs of polylines whose resampled rows stay within `budget` a run; a polyline that alone exceeds it is
    a run of its own.  out_offsets: the host copy of what the count phase wrote."""
    if budget < 1:
        raise ValueError("the row budget must be at least 1")
    S, cuts, a = len(out_offsets) - 1, [], 0
    while a < S:
        b = int(np.searchsorted(out_offsets, out_offsets[a] + budget, side="right")) - 1
        b = min(max(b, a + 1), S)
        cuts.append((a, b))
        a = b
    return cuts


def _resampled_runs(xy_d, offsets, spacing, row_budget):
    """Yields (a, b, out_xy, out_offsets) per run of polylines a .. b - 1: the whole batch is measured once (8 bytes a point), the
    offsets come back to the host, and every run is resampled by a call of its own whose output stays within the row budget."""
    import torch
    from . import ops
    dev = xy_d.device
    total = ops.polyline_resample_offsets(xy_d, torch.from_numpy(offsets).to(dev), spacing).cpu().numpy()
    for a, b in _cut_by_rows(total, row_budget):
        lo, hi = int(offsets[a]), int(offsets[b])
        if hi == lo:
            continue
        part = torch.from_numpy(offsets[a:b + 1] - lo).to(dev)
        out_xy, out_offsets = ops.polyline_resample(xy_d[lo:hi], part, spacing)
        yield a, b, out_xy, out_offsets


def resample_lines(lines, spacing=None, n_points=None, device=None, row_budget=None):
    """A list of (n, 2) absolute polylines -> each resampled along its arc length, float32: with `spacing` a point every `spacing`
    units and the end point (ceil(length / spacing) + 1 rows; an empty polyline stays empty), with `n_points` that many points
    equally spaced (an empty polyline gives n_points rows (0, 0)).  The rule of include/skf.h (Arc-length resampling), bit-equal
    to its host restatement; the ends are kept bit for bit.  Coordinates must be finite and within +-2^14: ValueError otherwise,
    before anything is copied to the device.  row_budget: the resampled rows one device call may produce (RESAMPLE_ROW_BUDGET):
    the batch is cut by the counts of a first pass over all of it."""
    lines, offsets, xy = _pack_lines(lines)
    spacing, n_points = _check_resample(xy, spacing, n_points)
    if len(xy) == 0:
        return [np.zeros((0 if n_points is None else n_points, 2), np.float32) for _ in lines]
    import torch
    from . import ops
    dev = _device(device)
    budget = RESAMPLE_ROW_BUDGET if row_budget is None else int(row_budget)
    out = [np.zeros((0, 2), np.float32)] * len(lines)
    with torch.cuda.device(dev):
        xy_d = torch.from_numpy(xy).to(dev)
        if n_points is not None:
            if budget < 1:
                raise ValueError("the row budget must be at least 1")
            step = max(1, budget // n_points)
            for a in range(0, len(lines), step):
                b = min(a + step, len(lines))
                lo, hi = int(offsets[a]), int(offsets[b])
                if hi == lo:
                    rows = np.zeros((b - a, n_points, 2), np.float32)
                else:
                    rows = ops.polyline_resample_n(xy_d[lo:hi], torch.from_numpy(offsets[a:b + 1] - lo).to(dev), n_points).cpu().numpy()
                out[a:b] = list(rows)
        else:
            for a, b, out_xy, out_offsets in _resampled_runs(xy_d, offsets, spacing, budget):
                rows, offs = out_xy.cpu().numpy(), out_offsets.cpu().numpy()
                out[a:b] = [rows[offs[i]:offs[i + 1]] for i in range(b - a)]
    return out


def simplify_lines(lines, epsilon, device=None, resample_spacing=None, row_budget=None):
    """A list of (n, 2) absolute polylines -> the kept points of each, in their own dtype.  The rule sees the points as float32.
    resample_spacing: every polyline is first resampled along its arc length at that spacing (resample_lines' rule and limits) and
    the resampled points go straight into the simplification on the device, under the new offsets; only the kept points come back,
    as float32.  The batch is cut so that one device call resamples at most row_budget rows (RESAMPLE_ROW_BUDGET), by the counts of
    a first pass over all of it: memory is bounded whatever the batch holds."""
    lines, offsets, xy = _pack_lines(lines)
    if resample_spacing is None:
        if len(xy) == 0:
            return [l.copy() for l in lines]
        import torch
        from . import ops
        dev = _device(device)
        with torch.cuda.device(dev):
            keep = ops.rdp_keep(torch.from_numpy(xy).to(dev), torch.from_numpy(offsets).to(dev), epsilon).cpu().numpy().astype(bool)
        return [l[keep[offsets[i]:offsets[i + 1]]] for i, l in enumerate(lines)]
    spacing, _ = _check_resample(xy, resample_spacing, None)
    out = [np.zeros((0, 2), np.float32)] * len(lines)
    if len(xy) == 0:
        return out
    import torch
    from . import ops
    dev = _device(device)
    budget = RESAMPLE_ROW_BUDGET if row_budget is None else int(row_budget)
    with torch.cuda.device(dev):
        for a, b, out_xy, out_offsets in _resampled_runs(torch.from_numpy(xy).to(dev), offsets, spacing, budget):
            keep = ops.rdp_keep(out_xy, out_offsets, epsilon).to(torch.bool)
            kept = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep, 0)])[out_offsets]
            rows, offs = out_xy[keep].cpu().numpy(), kept.cpu().numpy()
            out[a:b] = [rows[offs[i]:offs[i + 1]] for i in range(b - a)]
    return out


def quickdraw_lines(drawing):
    """The "drawing" field of a raw QuickDraw record, a list of strokes [[x...], [y...], [t...]] (the times are optional and
    unused) -> a list of float64 (n, 2) polylines.  Strokes without a point are left out."""
    lines = []
    for stroke in drawing:
        x, y = np.asarray(stroke[0], np.float64), np.asarray(stroke[1], np.float64)
        if x.shape != y.shape or x.ndim != 1:
            raise ValueError("a stroke must hold as many x as y")
        if len(x):
            lines.append(np.stack([x, y], axis=1))
    return lines


def scale_to_255(lines):
    """Align a drawing to the top-left corner and scale it uniformly, in float64, so that its larger extent is 255; a drawing of
    extent 0 is only aligned.  -> float32 polylines."""
    lines = [np.asarray(l, np.float64).reshape(-1, 2) for l in lines]
    pts = [l for l in lines if len(l)]
    if not pts:
        return [l.astype(np.float32) for l in lines]
    every = np.concatenate(pts, axis=0)
    lo = every.min(axis=0)
    extent = float((every.max(axis=0) - lo).max())
    if extent > 0:
        return [((l - lo) * (255.0 / extent)).astype(np.float32) for l in lines]
    return [(l - lo).astype(np.float32) for l in lines]


def drawing_to_stroke3(drawing, dtype=np.int16):
    """A list of (n, 2) absolute polylines -> one stroke-3 sketch (P, 3) of `dtype`: the positions rounded to integers (np.rint),
    one row per point as the offset from the point before it - across strokes too, the first from (0, 0) - and pen == 1 on the last
    point of every stroke.  Polylines without a point are left out; a drawing without a point gives (0, 3)."""
    lines = [np.rint(np.asarray(l, np.float64).reshape(-1, 2)) for l in drawing]
    lines = [l for l in lines if len(l)]
    if not lines:
        return np.zeros((0, 3), dtype=dtype)
    pos = np.concatenate(lines, axis=0)
    out = np.zeros((len(pos), 3), dtype=np.float64)
    out[0, :2] = pos[0]
    out[1:, :2] = pos[1:] - pos[:-1]
    out[np.cumsum([len(l) for l in lines]) - 1, 2] = 1
    info = np.iinfo(dtype) if np.issubdtype(np.dtype(dtype), np.integer) else None
    if info is not None and (out.min() < info.min or out.max() > info.max):
        raise ValueError("the offsets do not fit %s" % np.dtype(dtype).name)
    return out.astype(dtype)
