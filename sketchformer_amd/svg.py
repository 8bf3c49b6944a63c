"""SVG sketches as model input: a path parser on the host (xml.etree and re, no other dependency) and the device pipeline behind
it - flatten the curves (skf_path_flatten_*; include/skf.h has the rule, DESIGN.md section 3v the reasons), normalise, simplify
(skf_rdp_f32) - that turns TU-Berlin / Sketchy style files into stroke-3 sketches.  It stands where the reference has
utils/skt_tools.py: read_svg, which samples every path by its length through svgpathtools and simplifies with the rdp package.
The device functions have no CPU fallback; the parser is plain Python and numpy.

Conventions.  A subpath is a pair (ctrl, kind): ctrl (g, 4, 2) float64 holds the control points p0 .. p3 of g segments in absolute
coordinates, kind (g,) int32 is 1 for a cubic and 0 for a line (whose p1 = p0 and p2 = p3).  A drawing is a list of subpaths, each
with at least one segment: one stroke each.
"""
import math
import os
import re
import xml.etree.ElementTree as ET

import numpy as np

WORKING_SIZE = 1024.0          # the larger side of a drawing's working frame: inside simplify.RESAMPLE_MAX_COORD
FLATTEN_ROW_BUDGET = 1 << 24   # flattened rows one device call may produce (simplify.RESAMPLE_ROW_BUDGET)

_NUMBER = re.compile(r"[+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?")
_SEPARATOR = re.compile(r"[\s,]*")
_ARGS = {"M": 2, "L": 2, "H": 1, "V": 1, "C": 6, "S": 4, "Q": 4, "T": 2, "A": 7, "Z": 0}
ARC_PIECE = math.pi / 4        # an arc is cut into cubics of at most 45 degrees


# ---------------------------------------------------------------- path data
class _Scanner:
    def __init__(self, text):
        self.text, self.at = text, 0
        self.skip()

    def skip(self):
        self.at = _SEPARATOR.match(self.text, self.at).end()

    def done(self):
        return self.at >= len(self.text)

    def fail(self, what):
        raise ValueError("malformed path data at position %d: %s" % (self.at, what))

    def command(self):
        ch = self.text[self.at]
        if ch.upper() not in _ARGS:
            self.fail("expected a command, found %r" % ch)
        self.at += 1
        self.skip()
        return ch

    def more_numbers(self):
        return not self.done() and (self.text[self.at] in "+-." or self.text[self.at].isdigit())

    def number(self):
        m = _NUMBER.match(self.text, self.at)
        if m is None:
            self.fail("expected a number" + ("" if self.done() else ", found %r" % self.text[self.at]))
        self.at = m.end()
        self.skip()
        return float(m.group(0))

    def arc_flag(self):
        """a single 0 or 1, which need not be separated from what follows (`a1 1 0 01 10 10`)"""
        if self.done() or self.text[self.at] not in "01":
            self.fail("expected an arc flag (0 or 1)")
        flag = self.text[self.at] == "1"
        self.at += 1
        self.skip()
        return flag


def _line(p0, p3):
    return (p0, p0, p3, p3), 0


def _quadratic(p0, q, p3):
    """the cubic of the same curve (degree elevation)"""
    c1 = (p0[0] + 2.0 / 3.0 * (q[0] - p0[0]), p0[1] + 2.0 / 3.0 * (q[1] - p0[1]))
    c2 = (p3[0] + 2.0 / 3.0 * (q[0] - p3[0]), p3[1] + 2.0 / 3.0 * (q[1] - p3[1]))
    return (p0, c1, c2, p3), 1


def arc_segments(p0, rx, ry, rotation, large, sweep, p3):
    """An SVG elliptical arc from p0 to p3 as segments, by the SVG implementation notes: coincident ends give nothing, a zero radius
    a line; otherwise the centre parameterisation, radii that cannot reach scaled up, the sweep cut into equal pieces of at most 45
    degrees and every piece replaced by the cubic with k = 4/3 tan(theta / 4).  Such a piece leaves its arc by at most 4.25e-6 of
    the radius (measured in numpy at 45 degrees: 1 + 4.25e-6 at the worst parameter, 1 at the ends and the middle).  The ends of
    the arc are the given points bit for bit."""
    if p0 == p3:
        return []
    rx, ry = abs(rx), abs(ry)
    if rx == 0.0 or ry == 0.0:
        return [_line(p0, p3)]
    phi = math.radians(rotation % 360.0)
    cp, sp = math.cos(phi), math.sin(phi)
    dx, dy = (p0[0] - p3[0]) / 2.0, (p0[1] - p3[1]) / 2.0
    x1, y1 = cp * dx + sp * dy, -sp * dx + cp * dy
    lam = (x1 * x1) / (rx * rx) + (y1 * y1) / (ry * ry)
    if lam > 1.0:
        rx, ry = math.sqrt(lam) * rx, math.sqrt(lam) * ry
    num = rx * rx * ry * ry - rx * rx * y1 * y1 - ry * ry * x1 * x1
    den = rx * rx * y1 * y1 + ry * ry * x1 * x1
    co = math.sqrt(max(num / den, 0.0)) * (-1.0 if large == sweep else 1.0)
    cxp, cyp = co * rx * y1 / ry, -co * ry * x1 / rx
    cx = cp * cxp - sp * cyp + (p0[0] + p3[0]) / 2.0
    cy = sp * cxp + cp * cyp + (p0[1] + p3[1]) / 2.0
    theta = math.atan2((y1 - cyp) / ry, (x1 - cxp) / rx)
    delta = math.atan2((-y1 - cyp) / ry, (-x1 - cxp) / rx) - theta
    if sweep and delta < 0:
        delta += 2.0 * math.pi
    elif not sweep and delta > 0:
        delta -= 2.0 * math.pi
    pieces = max(1, int(math.ceil(abs(delta) / ARC_PIECE - 1e-9)))
    step = delta / pieces
    k = 4.0 / 3.0 * math.tan(step / 4.0)

    def point(a):          # the point of the ellipse at the angle a, and its derivative by the angle
        ca, sa = math.cos(a), math.sin(a)
        return ((cx + cp * rx * ca - sp * ry * sa, cy + sp * rx * ca + cp * ry * sa),
                (-cp * rx * sa - sp * ry * ca, -sp * rx * sa + cp * ry * ca))

    out, a, da = [], p0, point(theta)[1]
    for i in range(1, pieces + 1):
        b, db = point(theta + i * step)
        if i == pieces:
            b = p3
        out.append(((a, (a[0] + k * da[0], a[1] + k * da[1]), (b[0] - k * db[0], b[1] - k * db[1]), b), 1))
        a, da = b, db
    return out


def parse_path(d):
    """SVG path data -> a list of subpaths (ctrl (g, 4, 2) float64, kind (g,) int32), lines and cubics only.  The whole grammar:
    M m L l H h V v C c S s Q q T t A a Z z, implicit repeats (and the implicit lineto after a moveto), numbers such as
    `.5-.5e1`, arc flags written without separators, S / T reflection (the current point itself after a command that is no curve
    of their kind), a command after z starting from the subpath's start.  Z adds the closing line only when the pen is not at the
    start already.  Quadratics are degree-elevated and arcs become cubics (arc_segments).  A subpath that draws nothing (a lone
    moveto) is left out.  Malformed data raises ValueError naming the position."""
    sc = _Scanner(d)
    subpaths, segs = [], []
    cur = start = (0.0, 0.0)
    reflect, reflect_kind = None, None               # the last control point of the previous curve, and 'C' or 'Q'

    def close_subpath():
        if segs:
            subpaths.append((np.array([s[0] for s in segs], np.float64).reshape(-1, 4, 2), np.array([s[1] for s in segs], np.int32)))
            del segs[:]

    if not sc.done() and sc.text[sc.at] not in "Mm":
        sc.fail("path data must begin with a moveto")
    while not sc.done():
        where = sc.at
        letter = sc.command()
        cmd, rel = letter.upper(), letter.islower()
        if cmd == "Z":
            if cur != start:
                segs.append(_line(cur, start))
            close_subpath()
            cur, reflect_kind = start, None
            continue
        if not sc.more_numbers():
            sc.at = where
            sc.fail("the command %r has no arguments" % letter)
        first = True
        while first or sc.more_numbers():
            if cmd == "A":
                v = [sc.number(), sc.number(), sc.number(), sc.arc_flag(), sc.arc_flag(), sc.number(), sc.number()]
            else:
                v = [sc.number() for _ in range(_ARGS[cmd])]
            ox, oy = cur if rel else (0.0, 0.0)
            this_kind = None
            if cmd == "M" and first:
                close_subpath()
                cur = start = (ox + v[0], oy + v[1])
            elif cmd in "ML":
                end = (ox + v[0], oy + v[1])
                segs.append(_line(cur, end))
                cur = end
            elif cmd == "H":
                end = (ox + v[0], cur[1])
                segs.append(_line(cur, end))
                cur = end
            elif cmd == "V":
                end = (cur[0], oy + v[0])
                segs.append(_line(cur, end))
                cur = end
            elif cmd in "CS":
                if cmd == "C":
                    c1, v = (ox + v[0], oy + v[1]), v[2:]
                else:
                    c1 = (2.0 * cur[0] - reflect[0], 2.0 * cur[1] - reflect[1]) if reflect_kind == "C" else cur
                c2, end = (ox + v[0], oy + v[1]), (ox + v[2], oy + v[3])
                segs.append(((cur, c1, c2, end), 1))
                cur, reflect, this_kind = end, c2, "C"
            elif cmd in "QT":
                if cmd == "Q":
                    q, v = (ox + v[0], oy + v[1]), v[2:]
                else:
                    q = (2.0 * cur[0] - reflect[0], 2.0 * cur[1] - reflect[1]) if reflect_kind == "Q" else cur
                end = (ox + v[0], oy + v[1])
                segs.append(_quadratic(cur, q, end))
                cur, reflect, this_kind = end, q, "Q"
            else:                                    # A
                end = (ox + v[5], oy + v[6])
                segs.extend(arc_segments(cur, v[0], v[1], v[2], v[3], v[4], end))
                cur = end
            reflect_kind = this_kind
            first = False
    close_subpath()
    return subpaths


# ---------------------------------------------------------------- documents
_TRANSFORM = re.compile(r"([A-Za-z]+)\s*\(([^)]*)\)")
_LENGTH = re.compile(r"\s*(" + _NUMBER.pattern + r")\s*(?:px)?\s*$")
_SKIPPED_SUBTREES = ("defs", "clipPath", "mask", "pattern", "marker", "symbol")
_DRAWN = ("path", "line", "polyline", "polygon", "rect", "circle", "ellipse")
_WHITE = ("#fff", "#ffffff", "white")
IDENTITY = np.eye(3)


def parse_transform(text):
    """A transform attribute -> the 3 x 3 float64 matrix of the list, the leftmost transform outermost.  matrix, translate, scale,
    rotate(a [cx cy]), skewX, skewY; anything else in the list is passed over."""
    m = IDENTITY
    for name, args in _TRANSFORM.findall(text or ""):
        try:
            v = [float(x) for x in _NUMBER.findall(args)]
        except ValueError:
            continue
        t = None
        if name == "matrix" and len(v) == 6:
            t = np.array([[v[0], v[2], v[4]], [v[1], v[3], v[5]], [0, 0, 1]], np.float64)
        elif name == "translate" and len(v) in (1, 2):
            t = np.array([[1, 0, v[0]], [0, 1, v[1] if len(v) == 2 else 0.0], [0, 0, 1]], np.float64)
        elif name == "scale" and len(v) in (1, 2):
            t = np.diag([v[0], v[1] if len(v) == 2 else v[0], 1.0])
        elif name == "rotate" and len(v) in (1, 3):
            a = math.radians(v[0])
            r = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]], np.float64)
            if len(v) == 3:
                to, back = np.eye(3), np.eye(3)
                to[:2, 2], back[:2, 2] = (v[1], v[2]), (-v[1], -v[2])
                r = to @ r @ back
            t = r
        elif name == "skewX" and len(v) == 1:
            t = np.array([[1, math.tan(math.radians(v[0])), 0], [0, 1, 0], [0, 0, 1]], np.float64)
        elif name == "skewY" and len(v) == 1:
            t = np.array([[1, 0, 0], [math.tan(math.radians(v[0])), 1, 0], [0, 0, 1]], np.float64)
        if t is not None:
            m = m @ t
    return m


def _local(tag):
    return tag.rsplit("}", 1)[-1] if isinstance(tag, str) else ""


def _erased(el):
    """the reference's rule for Sketchy's erased strokes, slightly widened: a white stroke, as an attribute or inside style"""
    stroke = el.get("stroke")
    for part in (el.get("style") or "").split(";"):
        name, _, value = part.partition(":")
        if name.strip().lower() == "stroke":
            stroke = value
    return stroke is not None and stroke.strip().lower() in _WHITE


def _lengths(el, names, defaults):
    """The attributes as numbers (bare or px) -> a list, or None when one of them is written in another unit"""
    out = []
    for name, default in zip(names, defaults):
        raw = el.get(name)
        if raw is None:
            out.append(default)
            continue
        m = _LENGTH.match(raw)
        if m is None:
            return None
        out.append(float(m.group(1)))
    return out


def _points_path(raw, close):
    v = [float(x) for x in _NUMBER.findall(raw or "")]
    v = v[:len(v) - len(v) % 2]
    if len(v) < 4:
        return None
    return "M" + " ".join(repr(x) for x in v) + (" Z" if close else "")


def _ellipse_path(cx, cy, rx, ry):
    if not (rx > 0 and ry > 0):
        return None
    return "M%r %r A%r %r 0 1 1 %r %r A%r %r 0 1 1 %r %r Z" % (cx + rx, cy, rx, ry, cx - rx, cy, rx, ry, cx + rx, cy)


def _rect_path(el):
    v = _lengths(el, ("x", "y", "width", "height"), (0.0, 0.0, 0.0, 0.0))
    r = _lengths(el, ("rx", "ry"), (None, None))
    if v is None or r is None or not (v[2] > 0 and v[3] > 0):
        return None
    x, y, w, h = v
    rx, ry = r
    rx, ry = (ry if rx is None else rx), (rx if ry is None else ry)
    rx, ry = min(max(rx or 0.0, 0.0), w / 2.0), min(max(ry or 0.0, 0.0), h / 2.0)
    if rx == 0.0 or ry == 0.0:
        return "M%r %r H%r V%r H%r Z" % (x, y, x + w, y + h, x)
    return ("M%r %r H%r A%r %r 0 0 1 %r %r V%r A%r %r 0 0 1 %r %r H%r A%r %r 0 0 1 %r %r V%r A%r %r 0 0 1 %r %r Z"
            % (x + rx, y, x + w - rx, rx, ry, x + w, y + ry, y + h - ry, rx, ry, x + w - rx, y + h, x + rx, rx, ry, x, y + h - ry,
               y + ry, rx, ry, x + rx, y))


def _element_path(el, tag):
    """The path data of a drawable element, or None when it draws nothing that is understood"""
    if tag == "path":
        return el.get("d")
    if tag == "line":
        v = _lengths(el, ("x1", "y1", "x2", "y2"), (0.0, 0.0, 0.0, 0.0))
        return None if v is None else "M%r %r L%r %r" % tuple(v)
    if tag in ("polyline", "polygon"):
        return _points_path(el.get("points"), tag == "polygon")
    if tag == "rect":
        return _rect_path(el)
    if tag == "circle":
        v = _lengths(el, ("cx", "cy", "r"), (0.0, 0.0, 0.0))
        return None if v is None else _ellipse_path(v[0], v[1], v[2], v[2])
    if tag == "ellipse":
        v = _lengths(el, ("cx", "cy", "rx", "ry"), (0.0, 0.0, 0.0, 0.0))
        return None if v is None else _ellipse_path(*v)
    return None


def _root(source):
    if isinstance(source, bytes):
        return ET.fromstring(source)
    if isinstance(source, str) and source.lstrip().startswith("<"):
        return ET.fromstring(source)
    return ET.parse(os.fspath(source)).getroot()


def parse_svg(source):
    """An SVG document - a file path, bytes or text - -> a drawing: the subpaths of its path, line, polyline, polygon, rect (with
    rx / ry), circle and ellipse elements in document order, namespaced or not, after the transform of the element and of its g
    ancestors (composed in float64 and applied to the control points: an affine map commutes with Bezier evaluation).  An element
    whose stroke is white (#fff, #ffffff, white; as an attribute or inside style) is an erased stroke and is dropped, as is a
    subpath without a drawn segment.  Everything else - text, fills, style sheets, clip paths, use, lengths in units other than
    px - is passed over.  Malformed path data raises ValueError; XML that does not parse raises ValueError too."""
    try:
        root = _root(source)
    except ET.ParseError as e:
        raise ValueError("not well-formed XML: %s" % e)
    drawing = []

    def walk(el, matrix):
        tag = _local(el.tag)
        if tag in _SKIPPED_SUBTREES:
            return
        if tag == "g" or tag in _DRAWN:
            matrix = matrix @ parse_transform(el.get("transform"))
        if tag in _DRAWN and not _erased(el):
            d = _element_path(el, tag)
            if d:
                for ctrl, kind in parse_path(d):
                    drawing.append((ctrl @ matrix[:2, :2].T + matrix[:2, 2], kind))
        for child in el:
            walk(child, matrix)

    walk(root, IDENTITY)
    return drawing


# ---------------------------------------------------------------- the device pipeline
def working_frame(drawing):
    """A drawing with the bounding box of its control points moved to the origin and scaled, in float64, so that its larger side
    is WORKING_SIZE; a box of extent 0 is only moved.  The coordinates stay inside simplify.RESAMPLE_MAX_COORD and a flattening
    tolerance means the same whatever units the file used."""
    if not drawing:
        return []
    every = np.concatenate([c.reshape(-1, 2) for c, _ in drawing], axis=0)
    if not np.isfinite(every).all():
        raise ValueError("the control points must be finite")
    lo = every.min(axis=0)
    extent = float((every.max(axis=0) - lo).max())
    factor = WORKING_SIZE / extent if extent > 0 else 1.0
    return [((c - lo) * factor, k) for c, k in drawing]


def _pack_drawings(drawings):
    """-> (ctrl (G, 4, 2) float64, kind (G,) int32, path_offsets (S + 1) int64, drawing_paths (D + 1) int64: drawing i owns the
    subpaths drawing_paths[i] .. drawing_paths[i + 1] - 1)"""
    subpaths = [sp for d in drawings for sp in d]
    path_offsets = np.zeros(len(subpaths) + 1, np.int64)
    np.cumsum([len(k) for _, k in subpaths], out=path_offsets[1:])
    drawing_paths = np.zeros(len(drawings) + 1, np.int64)
    np.cumsum([len(d) for d in drawings], out=drawing_paths[1:])
    if subpaths:
        ctrl = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1, 4, 2) for c, _ in subpaths], axis=0))
        kind = np.ascontiguousarray(np.concatenate([np.asarray(k, np.int32).reshape(-1) for _, k in subpaths]))
    else:
        ctrl, kind = np.zeros((0, 4, 2), np.float64), np.zeros(0, np.int32)
    return ctrl, kind, path_offsets, drawing_paths


def _flattened_runs(drawings, tol, dev, row_budget):
    """Yields (a, b, out_xy, out_offsets, paths) per run of drawings a .. b - 1: the whole batch is counted once, the offsets come
    back to the host, and every run is flattened by a call of its own whose output stays within the row budget (a drawing that
    alone exceeds it is a run of its own).  paths: the run's slice of drawing_paths, counted from its first subpath."""
    import torch
    from . import ops, simplify
    ctrl, kind, path_offsets, drawing_paths = _pack_drawings(drawings)
    if len(kind) == 0:
        return
    ctrl_d, kind_d = torch.from_numpy(ctrl).to(dev), torch.from_numpy(kind).to(dev)
    budget = FLATTEN_ROW_BUDGET if row_budget is None else int(row_budget)
    total = ops.path_flatten_offsets(ctrl_d, kind_d, torch.from_numpy(path_offsets).to(dev), tol).cpu().numpy()
    for a, b in simplify._cut_by_rows(total[drawing_paths], budget):
        s0, s1 = int(drawing_paths[a]), int(drawing_paths[b])
        lo, hi = int(path_offsets[s0]), int(path_offsets[s1])
        if hi == lo:
            continue
        part = torch.from_numpy(path_offsets[s0:s1 + 1] - lo).to(dev)
        out_xy, out_offsets = ops.path_flatten(ctrl_d[lo:hi], kind_d[lo:hi], part, tol)
        yield a, b, out_xy, out_offsets, drawing_paths[a:b + 1] - s0


def flatten_paths(drawings, tol, device=None, row_budget=None):
    """A list of drawings -> per drawing a list of float32 (n, 2) polylines, one per subpath: the curves flattened on the device
    at `tol`, in the units of the control points as they are given (no working frame), by the rule of include/skf.h (Path
    flattening), bit-equal to its host restatement."""
    import torch
    from .preprocess import _device
    out = [[] for _ in drawings]
    if not any(len(d) for d in drawings):
        return out
    dev = _device(device)
    with torch.cuda.device(dev):
        for a, b, out_xy, out_offsets, paths in _flattened_runs(drawings, tol, dev, row_budget):
            rows, offs = out_xy.cpu().numpy(), out_offsets.cpu().numpy()
            for i in range(a, b):
                out[i] = [rows[offs[s]:offs[s + 1]] for s in range(int(paths[i - a]), int(paths[i - a + 1]))]
    return out


def _normalised(xy, row_drawing, n_drawings, scale):
    """The reference's normalisation on the device: per drawing the minimum and the maximum of the flattened float32 rows (exact
    and order-free), then ((x - min) / max_hw * 2 - 1) * scale as single float64 operations in that order, cast once to float32.
    A drawing of extent 0 is only aligned."""
    import torch
    index = row_drawing[:, None].expand(-1, 2).contiguous()
    lo = torch.full((n_drawings, 2), float("inf"), dtype=torch.float32, device=xy.device).scatter_reduce_(0, index, xy, "amin")
    hi = torch.full((n_drawings, 2), float("-inf"), dtype=torch.float32, device=xy.device).scatter_reduce_(0, index, xy, "amax")
    lo, hi = lo.double(), hi.double()
    max_hw = (hi - lo).max(dim=1).values
    moved = xy.double() - lo[row_drawing]
    side = max_hw[row_drawing][:, None]
    scale_d = torch.full((), float(scale), dtype=torch.float64, device=xy.device)
    two, one = torch.full_like(scale_d, 2.0), torch.full_like(scale_d, 1.0)
    full = ((moved / side) * two - one) * scale_d
    return torch.where(side > 0, full, moved).float()


def _stroke3(rows, kept_offsets, omit_first_point):
    """lines_to_strokes of the reference: the kept rows of one drawing (float32 absolute points) and the offsets of its strokes in
    them -> (n, 3) float32: differences taken in float64 and cast once, pen 1 on a stroke's last point."""
    if len(rows) == 0:
        return np.zeros((0, 3), np.float32)
    out = np.zeros((len(rows), 3), np.float64)
    out[:, :2] = rows
    out[1:, :2] -= rows[:-1].astype(np.float64)
    ends = np.unique(kept_offsets[1:]) - 1
    out[ends[ends >= 0], 2] = 1
    return out[1 if omit_first_point else 0:].astype(np.float32)


def svg_to_stroke3(sources, scale=100.0, epsilon=1.5, tol=0.0625, device=None, omit_first_point=True, row_budget=None):
    """SVG documents (paths, bytes, text, or drawings parse_svg returned) -> a list of (n, 3) float32 stroke-3 sketches, what the
    reference's read_svg returns for each: every drawing moved into its working frame on the host (working_frame), the whole batch
    flattened on the device at `tol` (in units of that frame, 1024 to the larger side), normalised to +-scale there as the
    reference normalises, simplified by skf_rdp_f32 at `epsilon`, and only the kept rows brought back.  A drawing without ink
    gives (0, 3).  row_budget: the flattened rows one device call may produce (FLATTEN_ROW_BUDGET); the batch is cut between
    drawings by the counts of a first pass over all of it.  Bit-equal to the host composition of the three rules."""
    import torch
    from . import ops
    from .preprocess import _device
    drawings = [working_frame(s if isinstance(s, list) else parse_svg(s)) for s in sources]
    out = [np.zeros((0, 3), np.float32) for _ in drawings]
    if not any(len(d) for d in drawings):
        return out
    dev = _device(device)
    with torch.cuda.device(dev):
        for a, b, xy, offs, paths in _flattened_runs(drawings, tol, dev, row_budget):
            paths_d = torch.from_numpy(np.ascontiguousarray(paths)).to(dev)
            drawing_rows = offs[paths_d]                                      # (b - a + 1): the rows of every drawing of the run
            row_drawing = torch.searchsorted(drawing_rows[1:].contiguous(), torch.arange(xy.shape[0], device=dev), right=True)
            norm = _normalised(xy, row_drawing, b - a, scale)
            keep = ops.rdp_keep(norm, offs, epsilon).to(torch.bool)
            kept = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep, 0)])[offs]
            rows, kept = norm[keep].cpu().numpy(), kept.cpu().numpy()
            for i in range(a, b):
                s0, s1 = int(paths[i - a]), int(paths[i - a + 1])
                out[i] = _stroke3(rows[kept[s0]:kept[s1]], kept[s0:s1 + 1] - kept[s0], omit_first_point)
    return out


def read_svg(svg_path, scale=100.0, draw_mode=False):
    """The reference's utils/skt_tools.py: read_svg: one SVG file -> its stroke-3 sketch, float32, the first point left out, inside
    +-scale with the larger side spanning 2 * scale, simplified at epsilon 1.5.  draw_mode is accepted and ignored."""
    return svg_to_stroke3([svg_path], scale=scale)[0]
