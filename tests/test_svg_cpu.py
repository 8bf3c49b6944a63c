"""The SVG parser of sketchformer_amd/svg.py on the CPU: the path grammar against hand-computed control points, the basic
shapes, transforms, erased strokes and the refusals.  Flattening where a test needs points is the host restatement
(tests/flatten_reference.py); tests/test_gpu_svg.py runs the device pipeline."""
import math
import os

import numpy as np
import pytest

import flatten_reference as fr
from sketchformer_amd import svg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svg")


def _segments(d):
    """the segments of every subpath of d as nested lists: [[(kind, p0, p1, p2, p3), ...], ...]"""
    return [[(int(k),) + tuple(tuple(pt) for pt in c.tolist()) for c, k in zip(ctrl, kind)] for ctrl, kind in svg.parse_path(d)]


def _line(a, b):
    a, b = tuple(map(float, a)), tuple(map(float, b))
    return (0, a, a, b, b)


def _same(a, b):
    assert len(a) == len(b)
    for (ca, ka), (cb, kb) in zip(a, b):
        assert np.array_equal(ka, kb) and ca.shape == cb.shape and np.allclose(ca, cb, rtol=0, atol=1e-12)


def test_lines_relative_forms_and_implicit_repeats():
    assert _segments("M10 10 20 20 30 10") == [[_line((10, 10), (20, 20)), _line((20, 20), (30, 10))]]
    assert _segments("m10 40 5 5 -5 5") == [[_line((10, 40), (15, 45)), _line((15, 45), (10, 50))]]
    assert _segments("M10 40 H40 V60 h-30 v-5") == [[_line((10, 40), (40, 40)), _line((40, 40), (40, 60)), _line((40, 60), (10, 60)),
                                                   _line((10, 60), (10, 55))]]
    assert _segments("M0 0 H10 20 V5 -5") == [[_line((0, 0), (10, 0)), _line((10, 0), (20, 0)), _line((20, 0), (20, 5)),
                                              _line((20, 5), (20, -5))]]
    assert _segments("M.5-.5e1 60,5.5e0") == [[_line((0.5, -5.0), (60.0, 5.5))]]
    assert _segments("M1 1 L2 2 M5 5 l1 0") == [[_line((1, 1), (2, 2))], [_line((5, 5), (6, 5))]]
    assert _segments("") == [] and _segments("M5 5") == [] and _segments("  M 5,5  ") == []


def test_closepath_and_what_follows_it():
    # Z closes with a line only when the pen is away from the start; a command after z starts from the start point
    assert _segments("M10 40 h30 v20 z l15 -8") == [[_line((10, 40), (40, 40)), _line((40, 40), (40, 60)), _line((40, 60), (10, 40))],
                                                    [_line((10, 40), (25, 32))]]
    assert _segments("M0 0 L5 0 L0 0 Z") == [[_line((0, 0), (5, 0)), _line((5, 0), (0, 0))]]
    assert _segments("M250 20 L260 30 Z Z M270 40 Z") == [[_line((250, 20), (260, 30)), _line((260, 30), (250, 20))]]
    assert _segments("M5 5 z") == []


def test_smooth_curves_equal_their_spelled_out_forms():
    _same(svg.parse_path("M100 100 c10 0 20 10 30 10 s20 10 30 0 S190 80 200 100"),
          svg.parse_path("M100 100 C110 100 120 110 130 110 C140 110 150 120 160 110 C170 100 190 80 200 100"))
    # after a command that is no cubic, S takes the current point as its first control point
    _same(svg.parse_path("M100 150 S120 130 140 150"), svg.parse_path("M100 150 C100 150 120 130 140 150"))
    _same(svg.parse_path("M0 0 Q5 5 10 0 S20 -5 30 0"), svg.parse_path("M0 0 Q5 5 10 0 C10 0 20 -5 30 0"))
    _same(svg.parse_path("M100 200 q20 -30 40 0 t40 0 T220 200"), svg.parse_path("M100 200 Q120 170 140 200 Q160 230 180 200 Q200 170 220 200"))
    _same(svg.parse_path("M100 250 T140 250"), svg.parse_path("M100 250 Q100 250 140 250"))    # the control point is the pen
    _same(svg.parse_path("M0 0 C1 2 3 4 5 5 T9 9"), svg.parse_path("M0 0 C1 2 3 4 5 5 Q5 5 9 9"))


def test_a_quadratic_is_degree_elevated():
    (ctrl, kind), = svg.parse_path("M0 0 Q30 60 90 0")
    assert kind.tolist() == [1] and np.allclose(ctrl[0], [(0, 0), (20, 40), (50, 40), (90, 0)], rtol=0, atol=1e-12)
    t = np.linspace(0, 1, 9)[:, None]
    quad = (1 - t) ** 2 * np.array([0, 0]) + 2 * (1 - t) * t * np.array([30, 60]) + t * t * np.array([90, 0])
    assert np.allclose(fr.bernstein(ctrl[0], t[:, 0]), quad, rtol=0, atol=1e-12)


def test_arcs_compact_flags_exact_ends_and_degenerate_forms():
    (ctrl, kind), = svg.parse_path("M10 10 a1 1 0 01 10 10")                 # flags 0 and 1, then 10 10; the radius is scaled up
    assert kind.tolist() == [1, 1, 1, 1] and ctrl[0, 0].tolist() == [10, 10] and ctrl[-1, 3].tolist() == [20, 20]
    assert np.array_equal(ctrl[1:, 0], ctrl[:-1, 3])
    r = math.hypot(5, 5)
    pts = fr.flatten_subpath(ctrl, kind, 0.001)
    assert np.abs(np.hypot(pts[:, 0] - 15, pts[:, 1] - 15) - r).max() <= 0.001 + 5e-6 * r + 2 ** -23 * 20
    assert (pts[:, 0] - pts[:, 1]).min() >= -1e-4                              # sweep 1 from (10, 10): the side where x >= y
    _same(svg.parse_path("M20 100 a25 25 0 01 50 0 a25,25 0 1050 0"), svg.parse_path("M20 100 A25 25 0 0 1 70 100 A25 25 0 1 0 120 100"))
    # exact ends whatever the radii and the rotation
    (ctrl, kind), = svg.parse_path("M40.1 280.3 A30 15 -30 1 0 90.7 260.9")
    assert ctrl[0, 0].tolist() == [40.1, 280.3] and ctrl[-1, 3].tolist() == [90.7, 260.9] and len(kind) >= 5
    # a quarter circle of radius 10 about (0, 0): one piece a 45 degrees, k = 4/3 tan(pi / 16)
    (ctrl, kind), = svg.parse_path("M10 0 A10 10 0 0 1 0 10")
    k = 4.0 / 3.0 * math.tan(math.pi / 16)
    h = math.sqrt(0.5)
    want = [[(10, 0), (10, 10 * k), (10 * h + 10 * k * h, 10 * h - 10 * k * h), (10 * h, 10 * h)],
            [(10 * h, 10 * h), (10 * h - 10 * k * h, 10 * h + 10 * k * h), (10 * k, 10), (0, 10)]]
    assert np.allclose(ctrl, want, rtol=0, atol=1e-12)
    # a zero radius is a line, coincident ends are nothing
    assert _segments("M20 160 A0 10 0 0 1 20 200") == [[_line((20, 160), (20, 200))]]
    assert _segments("M20 200 A10 10 30 1 1 20 200") == []
    assert _segments("M0 0 A5 5 0 1 1 0 0 L3 3") == [[_line((0, 0), (3, 3))]]


def test_a_circle_lies_on_its_circle():
    for r, tol in ((35.0, 0.05), (400.0, 0.25), (3.0, 0.01)):
        drawing = svg.parse_svg('<svg><circle cx="60" cy="-20" r="%r"/></svg>' % r)
        (ctrl, kind), = drawing
        assert kind.tolist() == [1] * 8 and np.array_equal(ctrl[0, 0], ctrl[-1, 3])      # closed without an extra line
        pts = fr.flatten_subpath(ctrl, kind, tol).astype(np.float64)
        err = np.abs(np.hypot(pts[:, 0] - 60, pts[:, 1] + 20) - r)
        mid = 0.5 * (pts[1:] + pts[:-1])
        err = max(err.max(), np.abs(np.hypot(mid[:, 0] - 60, mid[:, 1] + 20) - r).max())
        print("circle r %g tol %g: %d points, off the circle by %.3g" % (r, tol, len(pts), err))
        assert err <= tol + 5e-6 * r + 2 ** -23 * (60 + r)


def test_every_basic_shape():
    drawing = svg.parse_svg(os.path.join(GOLDEN, "shapes.svg"))
    assert [len(k) for _, k in drawing] == [1, 4, 5, 4, 12, 8, 8]          # line polyline polygon rect rounded-rect circle ellipse
    assert [int(k.sum()) for _, k in drawing] == [0, 0, 0, 0, 8, 8, 8]      # (the rect in cm, the text and the clip path are not ink)
    plain = svg.parse_svg('<svg><rect x="1" y="2" width="10" height="5"/><polygon points="0,0 4,0 4,3"/><ellipse rx="4" ry="2"/>'
                          '<rect width="8" height="6" rx="1"/><rect width="8" height="6" ry="50"/><rect width="0" height="6"/></svg>')
    assert len(plain) == 5
    assert plain[0][0][:, 0].tolist() == [[1, 2], [11, 2], [11, 7], [1, 7]] and plain[0][0][-1, 3].tolist() == [1, 2]
    assert plain[1][0][:, 3].tolist() == [[4, 0], [4, 3], [0, 0]]
    assert plain[2][0][0, 0].tolist() == [4, 0] and plain[2][0][3, 3].tolist() == [-4, 0]
    assert plain[3][0][0, 0].tolist() == [1, 0] and len(plain[3][1]) == 12                 # rx alone: ry = rx
    assert plain[4][0][0, 0].tolist() == [4, 0] and plain[4][0][0, 3].tolist() == [4, 0]   # ry 50 -> rx = ry, both clamped to w/2, h/2


def test_transforms_compose_like_a_hand_written_matrix():
    t20 = math.tan(math.radians(20))
    c15, s15 = math.cos(math.radians(15)), math.sin(math.radians(15))
    translate = np.array([[1, 0, 20], [0, 1, 10], [0, 0, 1.0]])
    scale = np.array([[1.5, 0, 0], [0, 0.75, 0], [0, 0, 1.0]])
    skew = np.array([[1, t20, 0], [0, 1, 0], [0, 0, 1.0]])
    rotate = np.array([[c15, -s15, 165 - 165 * c15 + 145 * s15], [s15, c15, 145 - 165 * s15 - 145 * c15], [0, 0, 1.0]])
    assert np.allclose(svg.parse_transform("translate(20 10) scale(1.5,0.75)skewX(20)"), translate @ scale @ skew, rtol=0, atol=1e-12)
    assert np.allclose(svg.parse_transform("rotate(15 165 145)"), rotate, rtol=0, atol=1e-12)
    assert np.allclose(svg.parse_transform("matrix(1 2 3 4 5 6) skewY(45) scale(2) translate(3) bogus(1)"),
                       np.array([[1, 3, 5], [2, 4, 6], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [1, 1, 0], [0, 0, 1.0]]) @ np.diag([2, 2, 1.0])
                       @ np.array([[1, 0, 3], [0, 1, 0], [0, 0, 1.0]]), rtol=0, atol=1e-12)
    drawing = svg.parse_svg(os.path.join(GOLDEN, "shapes.svg"))
    # the circle: under translate, scale and skewX; the rounded rect: under translate, scale and its own rotate
    raw_circle, = svg.parse_svg('<svg><circle cx="60" cy="230" r="35"/></svg>')
    m = translate @ scale @ skew
    assert np.allclose(drawing[5][0], raw_circle[0] @ m[:2, :2].T + m[:2, 2], rtol=0, atol=1e-9)
    raw_rect, = svg.parse_svg('<svg><rect x="120" y="120" width="90" height="50" rx="12" ry="20"/></svg>')
    m = translate @ scale @ rotate
    assert np.allclose(drawing[4][0], raw_rect[0] @ m[:2, :2].T + m[:2, 2], rtol=0, atol=1e-9)
    # the line sits under the outer translate alone
    assert np.allclose(drawing[0][0][0, [0, 3]], [(20, 10), (140, 50)], rtol=0, atol=1e-12)
    # TU-Berlin style: a matrix on the group
    curves = svg.parse_svg(os.path.join(GOLDEN, "curves.svg"))
    assert np.allclose(curves[0][0][0, 0], (0.8 * 211.3 - 40.5, 0.8 * 160.2 + 12.25), rtol=0, atol=1e-12)
    assert [len(k) for _, k in curves] == [5, 1, 1, 1, 8, 1, 1]


def test_an_affine_map_commutes_with_the_curve():
    (ctrl, _), = svg.parse_path("M0 0 C10 40 60 -20 80 30")
    m = svg.parse_transform("rotate(33) skewX(10) translate(4 5) scale(2 0.5)")
    t = np.linspace(0, 1, 17)
    mapped = fr.bernstein(ctrl[0] @ m[:2, :2].T + m[:2, 2], t)
    assert np.allclose(mapped, fr.bernstein(ctrl[0], t) @ m[:2, :2].T + m[:2, 2], rtol=0, atol=1e-10)


def test_the_erased_path_is_absent():
    drawing = svg.parse_svg(os.path.join(GOLDEN, "erased.svg"))
    assert [len(k) for _, k in drawing] == [2, 3, 1]
    every = np.concatenate([c.reshape(-1, 2) for c, _ in drawing])
    assert every.min() >= 20 and every[:, 0].max() <= 600 and every[:, 1].max() <= 460      # nothing of the white strokes' extent
    for stroke in ('stroke="#fff"', 'stroke="#FFF"', 'stroke="White"', 'stroke=" #ffffff "', 'style="stroke:#fff"',
                   'stroke="#000" style="fill:none;stroke : WHITE"'):
        assert svg.parse_svg('<svg><path %s d="M0 0 L9 9"/></svg>' % stroke) == [], stroke
    for stroke in ('stroke="#ffe"', 'fill="#fff"', 'style="fill:#fff"', 'stroke="#fff" style="stroke:#000"'):
        assert len(svg.parse_svg('<svg><path %s d="M0 0 L9 9"/></svg>' % stroke)) == 1, stroke


def test_sources_namespaces_and_what_is_ignored(tmp_path):
    text = '<svg xmlns="http://www.w3.org/2000/svg"><g><path d="M0 0 L5 5"/></g><text>x</text><use href="#a"/><path d="M3 3"/></svg>'
    path = tmp_path / "one.svg"
    path.write_text(text)
    for source in (text, text.encode(), str(path), path, text.replace(' xmlns="http://www.w3.org/2000/svg"', "")):
        drawing = svg.parse_svg(source)
        assert len(drawing) == 1 and drawing[0][0].dtype == np.float64 and drawing[0][1].dtype == np.int32
        assert drawing[0][0].shape == (1, 4, 2) and drawing[0][0][0, 3].tolist() == [5, 5]
    assert svg.parse_svg("<svg/>") == []
    grammar = svg.parse_svg(os.path.join(GOLDEN, "grammar.svg"))
    assert [len(k) for _, k in grammar] == [2, 4, 2, 1, 3, 1, 3, 3, 8, 5, 2, 6]


@pytest.mark.parametrize("d,position", [("L10 10", 0), ("M10 10 L20", 10), ("M0 0 X5 5", 5), ("M0 0 L1 1 C1 2 3", 16), ("M0 0 A5 5 0 2 1 9 9", 12),
                                        ("M0 0 L", 5), ("M0 0 L1 e5", 8), ("10 10", 0)])
def test_malformed_path_data_names_the_position(d, position):
    with pytest.raises(ValueError, match="position %d:" % position):
        svg.parse_path(d)
    with pytest.raises(ValueError, match="position %d:" % position):
        svg.parse_svg('<svg><path d="%s"/></svg>' % d)


def test_malformed_documents_and_frames():
    with pytest.raises(ValueError, match="XML"):
        svg.parse_svg("<svg><path d='M0 0'></svg>")
    with pytest.raises(ValueError, match="finite"):
        svg.working_frame([(np.full((1, 4, 2), np.inf), np.zeros(1, np.int32))])
    framed = svg.working_frame(svg.parse_svg('<svg><path d="M100 50 L300 50 L300 100"/></svg>'))
    assert framed[0][0][:, 3].tolist() == [[1024.0, 0.0], [1024.0, 256.0]] and framed[0][0][0, 0].tolist() == [0.0, 0.0]
    dot = svg.working_frame(svg.parse_svg('<svg><path d="M7 7 L7 7"/></svg>'))
    assert not dot[0][0].any() and svg.working_frame([]) == []
