"""Sketches as images: the device rasterizer (skf_raster.hip through ops.sketch_points / ops.rasterize / ops.raster_overlap)
behind the calls an evaluation needs - render a batch, lay a reconstruction over its original, score the overlap - and the host
helpers that turn the images into a PNG.  The reference draws through utils/sketch.py (svgwrite -> svglib, one sketch at a
time); here a sketch is a (H, W) float32 coverage image on the device, ink 1 and paper 0.  DESIGN.md section 3l."""
import numpy as np

KINDS = ('stroke3', 'stroke5', 'tokens')
UNIT_FRAME = (-1.0, -1.0, 1.0, 1.0)


def _size(size):
    if isinstance(size, (int, np.integer)):
        size = (size, size)
    H, W = (int(v) for v in size)
    if H < 1 or W < 1:
        raise ValueError("size must be (H, W) with H, W >= 1 (got %r)" % (size,))
    return H, W


def _check_style(size, line_width, margin):
    H, W = _size(size)
    if not line_width > 0:
        raise ValueError("line_width must be positive (got %r)" % (line_width,))
    if margin < 0 or 2 * margin >= min(H, W):
        raise ValueError("margin must be >= 0 and 2 * margin < min(H, W) (got %r for %d x %d)" % (margin, H, W))
    return H, W


def pack_stroke3(sketches):
    """A list of ragged (n_i, 3) stroke-3 arrays -> ((B, T, 3) float32 zero-padded, (B,) int32 lengths), T = the longest (>= 1)."""
    rows = [np.asarray(s, dtype=np.float32).reshape(-1, 3) for s in sketches]
    if not rows:
        raise ValueError("no sketches to pack")
    T = max(1, max(len(r) for r in rows))
    out = np.zeros((len(rows), T, 3), dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int32)


def _host_points(sketches, tokenizer):
    """Tokens of a tokenizer that is neither the dictionary nor the grid tokenizer (the synthetic loader's): decoded by its own
    decode_single on the host, summed in float64, handed to the rasterizer as points."""
    dec = [np.asarray(tokenizer.decode_single(np.asarray(s).reshape(-1)), dtype=np.float64).reshape(-1, 3) for s in sketches]
    T = max(1, max(len(d) for d in dec))
    B = len(dec)
    xy, pen = np.zeros((B, T, 2), np.float32), np.zeros((B, T), np.uint8)
    n, bounds = np.zeros(B, np.int32), np.zeros((B, 4), np.float32)
    for i, d in enumerate(dec):
        if len(d):
            p = np.cumsum(d[:, :2], axis=0).astype(np.float32)
            xy[i, :len(d)], pen[i, :len(d)], n[i] = p, d[:, 2] == 1, len(d)
            bounds[i] = np.r_[p.min(0), p.max(0)]
    return xy, pen, n, bounds


def points(sketches, kind='stroke3', tokenizer=None, lengths=None, device=None):
    """-> (xy, pen, n_points, bounds) device tensors (ops.sketch_points).  sketches: a numpy array or device tensor of the kind's
    shape - 'stroke3' (B, T, 3) with lengths (default: all T rows), or a list of ragged (n, 3) arrays; 'stroke5' (B, T, 5);
    'tokens' (B, L) ids, read with the tokenizer: its centres for the dictionary Tokenizer, its resolution for the GridTokenizer;
    any other tokenizer decodes on the host with its own decode_single."""
    import torch
    from . import ops
    if kind not in KINDS:
        raise ValueError("kind must be one of %s (got %r)" % (KINDS, kind))
    if kind == 'tokens' and tokenizer is None:
        raise ValueError("kind='tokens' needs the tokenizer that made the ids")
    dev = torch.device("cuda") if device is None else torch.device(device)
    if torch.is_tensor(sketches) and sketches.is_cuda:
        dev = sketches.device

    def dev_tensor(a, dtype):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=dev, dtype=dtype).contiguous()

    if kind == 'stroke3':
        if isinstance(sketches, (list, tuple)):
            if lengths is not None:
                raise ValueError("a list of ragged sketches carries its own lengths")
            sketches, lengths = pack_stroke3(sketches)
        data = dev_tensor(sketches, torch.float32)
        if data.dim() != 3 or data.shape[2] != 3:
            raise ValueError("stroke3 sketches must be (B, T, 3) (got %r)" % (tuple(data.shape),))
        if lengths is None:
            lengths = np.full(data.shape[0], data.shape[1], dtype=np.int32)
        return ops.sketch_points(data, 'stroke3', lengths=dev_tensor(lengths, torch.int32))
    if kind == 'stroke5':
        data = dev_tensor(sketches, torch.float32)
        if data.dim() != 3 or data.shape[2] != 5:
            raise ValueError("stroke5 sketches must be (B, T, 5) (got %r)" % (tuple(data.shape),))
        return ops.sketch_points(data, 'stroke5')
    if not torch.is_tensor(sketches):
        sketches = np.asarray(sketches)
    if sketches.ndim == 3 and sketches.shape[2] == 1:
        sketches = sketches[:, :, 0]                              # (N, L, 1) token columns of the file loaders
    if sketches.ndim != 2:
        raise ValueError("token sketches must be (B, L) (got %r)" % (tuple(sketches.shape),))
    if hasattr(tokenizer, 'centers'):
        centers = dev_tensor(np.asarray(tokenizer.centers), torch.float32)
        return ops.sketch_points(dev_tensor(sketches, torch.int64), 'dict_tokens', centers=centers)
    if hasattr(tokenizer, 'resolution'):
        return ops.sketch_points(dev_tensor(sketches, torch.int64), 'grid_tokens', resolution=int(tokenizer.resolution))
    host = sketches.cpu().numpy() if torch.is_tensor(sketches) else sketches
    xy, pen, n, bounds = _host_points(host, tokenizer)
    return (dev_tensor(xy, torch.float32), dev_tensor(pen, torch.uint8), dev_tensor(n, torch.int32), dev_tensor(bounds, torch.float32))


def render(sketches, kind='stroke3', tokenizer=None, size=(64, 64), line_width=1.5, margin=2.0, frame='fit', return_frames=False,
           lengths=None):
    """Draw B sketches into (B, H, W) float32 coverage images on the device.  frame: 'fit' = every sketch into its own bounds,
    'unit' = the box (-1, -1, 1, 1), or a (B, 4) tensor / array of boxes (x0, y0, x1, y1) - what return_frames=True hands back, so
    that a second batch can be drawn into the frames of the first."""
    import torch
    from . import ops
    H, W = _check_style(size, line_width, margin)
    if isinstance(frame, str) and frame not in ('fit', 'unit'):
        raise ValueError("frame must be 'fit', 'unit' or a (B, 4) tensor of boxes (got %r)" % (frame,))
    xy, pen, n, bounds = points(sketches, kind, tokenizer, lengths)
    B = xy.shape[0]
    if isinstance(frame, str):
        frames = bounds if frame == 'fit' else torch.tensor([UNIT_FRAME] * B, dtype=torch.float32, device=xy.device)
    else:
        frames = frame if torch.is_tensor(frame) else torch.from_numpy(np.ascontiguousarray(frame))
        frames = frames.to(device=xy.device, dtype=torch.float32).contiguous()
        if tuple(frames.shape) != (B, 4):
            raise ValueError("frame must hold one box (x0, y0, x1, y1) per sketch: (%d, 4), got %r" % (B, tuple(frames.shape)))
    images = ops.rasterize(xy, pen, n, frames, (H, W), line_width, margin)
    return (images, frames) if return_frames else images


def iou_from_sums(sums):
    """(B, 2) = (sum min, sum max) -> sum min / sum max per pair, 1.0 where both images are blank (sum max == 0).  numpy in,
    numpy out; a tensor in, a tensor out."""
    if isinstance(sums, np.ndarray):
        num, den = sums[:, 0], sums[:, 1]
        return np.where(den > 0, num / np.where(den > 0, den, 1), 1).astype(sums.dtype)
    import torch
    num, den = sums[:, 0], sums[:, 1]
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.ones_like(den))


def soft_iou(a, b):
    """Soft intersection over union of two stacks of coverage images on the device: sum min(a, b) / sum max(a, b) per pair (B,),
    1.0 when both are blank.  The sums come from ops.raster_overlap in a fixed order: identical images give exactly 1."""
    from . import ops
    return iou_from_sums(ops.raster_overlap(a, b))


def render_pair_iou(originals, reconstructions, kind='stroke3', tokenizer=None, size=(64, 64), line_width=1.5, margin=2.0,
                    lengths=None, recon_lengths=None):
    """Every reconstruction drawn into ITS ORIGINAL's frame (the original fitted to the canvas) -> (original images,
    reconstruction images, soft IoU (B,)), all on the device."""
    a, frames = render(originals, kind, tokenizer, size, line_width, margin, 'fit', True, lengths)
    b = render(reconstructions, kind, tokenizer, size, line_width, margin, frames, False, recon_lengths)
    return a, b, soft_iou(a, b)


# ---------------------------------------------------------------- host numpy: images -> a picture file
def to_uint8(images):
    """Coverage in [0, 1] -> uint8 with dark ink on white paper (255 = paper, 0 = full ink)."""
    if hasattr(images, 'detach'):
        images = images.detach().cpu().numpy()
    cov = np.clip(np.nan_to_num(np.asarray(images, dtype=np.float64)), 0.0, 1.0)
    return np.rint(255.0 * (1.0 - cov)).astype(np.uint8)


def contact_sheet(images, cols=6, pad=2, fill=255):
    """(N, H, W) images -> one (rows * (H + pad) + pad, cols * (W + pad) + pad) array, row-major, `fill` between and behind."""
    if hasattr(images, 'detach'):
        images = images.detach().cpu().numpy()
    images = np.asarray(images)
    if images.ndim != 3 or len(images) < 1:
        raise ValueError("contact_sheet takes a non-empty (N, H, W) stack (got %r)" % (images.shape,))
    cols, pad = int(cols), int(pad)
    if cols < 1 or pad < 0:
        raise ValueError("cols must be >= 1 and pad >= 0")
    N, H, W = images.shape
    rows = (N + cols - 1) // cols
    sheet = np.full((rows * (H + pad) + pad, cols * (W + pad) + pad), fill, dtype=images.dtype)
    for k in range(N):
        r, c = divmod(k, cols)
        y, x = pad + r * (H + pad), pad + c * (W + pad)
        sheet[y:y + H, x:x + W] = images[k]
    return sheet


def interlace(a, b):
    """(N, H, W), (N, H, W) -> (2 N, H, W): a[0], b[0], a[1], b[1], ... (the order of the reference's build_interlaced_grid_list)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError("interlace takes two stacks of one shape")
    out = np.empty((2 * a.shape[0],) + a.shape[1:], dtype=a.dtype)
    out[0::2], out[1::2] = a, b
    return out


def save_png(path, array):
    """Write a (H, W) uint8 grey image as a PNG with what is installed: matplotlib's imsave, else PIL."""
    array = np.asarray(array)
    if array.ndim != 2 or array.dtype != np.uint8:
        raise ValueError("save_png takes a (H, W) uint8 array")
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
        plt.imsave(path, array, cmap="gray", vmin=0, vmax=255, format="png")
    except ImportError:
        from PIL import Image
        Image.fromarray(array, mode="L").save(path, format="PNG")
    return path
