"""do_quantsmooth on PyTorch device tensors: the device-resident job route of include/jpegqs_hip.h
(qs_hip_do_quantsmooth_device) for coefficients that already live on the GPU.

    res = torch_qs.quantsmooth_(coefs, quants, flags, niter, hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3,
                                image_size=(1920, 1080))
    stop = int(res["stop"])          # the reference's return value (reading it synchronises)

Each coefficient array is a contiguous int16 CUDA tensor of shape (hblk, wblk, 64), rewritten in place.  The job is
enqueued on torch.cuda.current_stream() with no host synchronisation and no allocation outside torch's allocator, so
it can be captured into a torch.cuda.graph: run it once outside the capture (that prepares the workspace), then
capture a call that passes the same `workspace=`.

    res = torch_qs.quantsmooth_batch_([dict(coefs=..., quants=..., hsamp=..., ...), ...], flags, niter)
    stops = res["stop"]              # one int32 per image; res["images"][i] has image i's coef_up, quants, ...

runs many images in one call, their planes sharing kernel launches (qs_hip_do_quantsmooth_device_batch).

    px = torch_qs.decode(coefs, quants, hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3, image_size=(1920, 1080),
                         result=res)   # uint8 (H, W, C): what libjpeg 9 decodes from the smoothed arrays

decodes coefficient tensors to pixels on the device (qs_hip_decode_device_batch), after smoothing or on their own.

    data = torch_qs.encode(coefs, quants, hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3, image_size=(1920, 1080),
                           result=res)   # bytes: the JPEG file libjpeg 9 writes from the smoothed arrays

entropy-codes them on the device (qs_hip_encode_device_batch); encode_scan leaves the segment in device memory, and

    r = torch_qs.encode_file(coefs, quants, hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3, image_size=(1920, 1080),
                             result=res)   # r["file"][:r["len"]]: the whole file with optimized tables, in device memory

builds the optimal Huffman tables and the whole file on the device (qs_hip_encode_device_batch_files), capturable.

    im = torch_qs.read(data)          # data: the bytes of a JPEG file with restart intervals, on the host or the device

reads a file's scan into device coefficient tensors (qs_hip_read_device_batch, one lane per restart interval): the image
dict the three calls above take.  A progressive file (SOF2) goes to read_progressive (qs_hip_read_prog_device_batch: one
lane per restart interval of one scan, one decode launch per level of the script), also through read / read_batch.

    im = torch_qs.compress(pixels, quality=85, hsamp=[2, 1, 1], vsamp=[2, 1, 1])   # pixels: uint8 (H, W, 3) on the device

compresses pixels into the same image dict (qs_hip_compress_device_batch): libjpeg 9's jpeg_write_scanlines with
JDCT_ISLOW and either chroma downsampling -- downsampling="box" (do_fancy_downsampling = FALSE, the default here) or
downsampling="dct" (libjpeg 9's own default: 2x chroma through 16-point scaled forward DCTs).

torch is imported on first use only: importing the package does not need it."""
from __future__ import annotations

from functools import partial

import numpy as np

from .hipqs import HipQS

_HIP = None


def _hip() -> HipQS:
    global _HIP
    if _HIP is None:
        _HIP = HipQS()
    return _HIP


class Workspace:
    """device workspace of one job geometry: a torch uint8 tensor plus what it was prepared for (decode and
    decode_batch also take an empty Workspace() and fill it in place)"""

    def __init__(self, buf=None, key=None):
        self.buf, self.key = buf, key
        self.headers = None          # read_batch: the parsed headers of the files it was prepared with
        self.files = None            # encode_file_batch: the frames' device bytes and the scratch (a captured graph refers to them)

    @property
    def nbytes(self) -> int:
        return 0 if self.buf is None else int(self.buf.numel())


def _key(job, flags, niter):
    """what the workspace layout and its constants depend on: everything but the array addresses"""
    from .hipqs import Job
    g = Job.from_buffer_copy(job)
    for ci in range(4):
        g.coef[ci] = None
    g.coef_up[0] = g.coef_up[1] = None
    return (bytes(g), int(flags), int(niter))


def _check_tensors(coefs, torch, who="quantsmooth_"):
    if not isinstance(coefs, (list, tuple)) or not 1 <= len(coefs) <= 4:
        raise ValueError(f"{who}: coefs must be a list of 1..4 tensors")
    dev = None
    for ci, t in enumerate(coefs):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: component {ci} is not a torch.Tensor")
        if t.dtype != torch.int16:
            raise TypeError(f"{who}: component {ci} has dtype {t.dtype}, expected torch.int16")
        if t.dim() != 3 or t.shape[2] != 64 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: component {ci} has shape {tuple(t.shape)}, expected (hblk, wblk, 64)")
        if not t.is_contiguous():
            raise ValueError(f"{who}: component {ci} is not contiguous")
        if not t.is_cuda:
            raise ValueError(f"{who}: component {ci} is on {t.device}, expected a CUDA (HIP) device tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{who}: component {ci} is on {t.device}, component 0 on {dev}")
    return dev


def _check_quants(quants, n, who="quantsmooth_"):
    if len(quants) != n:
        raise ValueError(f"{who}: one quant table (or None) per component")
    qs = [None if q is None else np.asarray(q, dtype=np.int64).reshape(-1) for q in quants]
    for ci, q in enumerate(qs):
        if q is not None and (q.size != 64 or q.min() < 0 or q.max() > 0xFFFF):
            raise ValueError(f"{who}: quant table {ci} must be 64 values in 0..65535")
    return qs


def _device_job(hip, coefs, quants, **kw):
    """the qs_hip_job over coefficient tensors (kw: HipQS.device_job's keywords)"""
    return hip.device_job([t.data_ptr() for t in coefs], [tuple(t.shape[:2]) for t in coefs], quants, **kw)


def _prepared(workspace, key, total, dev, prepare, who, same, in_place=True):
    """The workspace step of every stage: `workspace` as it is when it was prepared for `key`, else prepared for it -- by
    prepare(address, bytes, stream) on dev's current stream, in a buffer of at least `total` bytes -- and keyed.  The key
    is what the layout and its constants depend on, everything but the array addresses; it starts with the stage's tag,
    so a workspace that comes from another stage is prepared again.  Preparing synchronises, so inside a graph capture it
    is refused; `same` words what the earlier call must have shared ("on the same geometry and tables (workspace=...)").

    A buffer that is too small or on another device is replaced in one of two ways.  in_place, every stage but the
    smoothing: the passed object gets the new buffer, and None stands for an empty Workspace() -- decode() and the other
    single-image forms return no dict that could carry a new object.  Not in_place, quantsmooth_ and quantsmooth_batch_:
    the passed object stays as it was, and a new Workspace is returned for the result dict to carry."""
    import torch
    if workspace is None and in_place:
        workspace = Workspace()
    if workspace is None or workspace.key != key:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: inside a graph capture the workspace must come from an earlier call {same}: "
                               f"preparing one synchronises")
        if workspace is None or workspace.buf is None or workspace.nbytes < total or workspace.buf.device != dev:
            buf = torch.empty(max(1, total), dtype=torch.uint8, device=dev)
            if in_place:
                workspace.buf = buf
            else:
                workspace = Workspace(buf)
        prepare(workspace.buf.data_ptr(), workspace.nbytes, torch.cuda.current_stream(dev).cuda_stream)
        workspace.key = key
    return workspace


def _check_list(images, who):
    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError(f"{who}: images must be a non-empty list of dicts")


def _images_on_one_device(images, result, who, needs, one, torch):
    """what the batch calls check of their images: a non-empty list of dicts that hold `needs`, all on one device, and
    `result` -- a smoothing result or None -- with one entry per image and its stop tensor on that device.
    one(i, image, the result's entry or None) checks image i as its stage requires, keeps what the stage needs of it and
    returns its device -> (the device, the stop tensor or None)"""
    _check_list(images, who)
    if result is not None and len(result["images"]) != len(images):
        raise ValueError(f"{who}: result holds {len(result['images'])} images, the batch {len(images)}")
    dev, keys, entries = None, set(needs), [None] * len(images) if result is None else result["images"]
    for i, (im, res) in enumerate(zip(images, entries)):
        if not isinstance(im, dict) or not im.keys() >= keys:
            raise ValueError(f"{who}: image {i} must be a dict with {' and '.join(needs)}")
        d = one(i, im, res)
        if dev is None:
            dev = d
        elif d != dev:
            raise ValueError(f"{who}: image {i} is on {d}, image 0 on {dev}")
    stop = None
    if result is not None:
        stop = result["stop"]
        _check_stop(stop, len(images), dev, who, torch)
    return dev, stop


def _batch_result(result):
    """a single image's smoothing result as the result of a batch of one"""
    return None if result is None else dict(stop=result["stop"], images=[result])


def _outs_of(out):
    return None if out is None else [out]


def _enqueue(jobs, tables, dev, flags, niter, workspace, who, single):
    """what quantsmooth_ (single: the single-job calls) and quantsmooth_batch_ share: the workspace, prepared outside
    any capture when the jobs changed; the replacement chroma tensors; the run on the current stream; what it reports"""
    import torch
    hip = _hip()
    if single:
        arg, prepare, run = jobs[0], hip.device_job_prepare, hip.do_quantsmooth_device
        per = [hip.device_job_info(arg, flags, niter)]
        total = per[0]["workspace_bytes"]
    else:
        arg, prepare, run = jobs, hip.device_batch_prepare, hip.do_quantsmooth_device_batch
        per, total = hip.device_batch_info(jobs, flags, niter)
    key = (single,) + tuple(_key(job, flags, niter) for job in jobs)     # (a job alone is laid out unlike a batch of one)
    workspace = _prepared(workspace, key, total, dev,
                          lambda ptr, nbytes, stream: prepare(arg, flags, niter, ptr, nbytes, stream), who,
                          f"of the same {'job' if single else 'batch'} (workspace=res['workspace'])", in_place=False)
    stream = torch.cuda.current_stream(dev)
    ups = []
    for job, inf in zip(jobs, per):
        up = None
        if inf["up_wblk"] > 0:
            up = [torch.empty((inf["up_hblk"], inf["up_wblk"], 64), dtype=torch.int16, device=dev) for _ in range(2)]
            job.coef_up[0], job.coef_up[1] = up[0].data_ptr(), up[1].data_ptr()
        ups.append(up)
    stop = torch.empty(len(jobs), dtype=torch.int32, device=dev)
    run(arg, flags, niter, workspace.buf.data_ptr(), workspace.nbytes, stop.data_ptr(), stream.cuda_stream)
    out = []
    for job, qs, up in zip(jobs, tables, ups):
        qout = [None if q is None else np.array(job.quant[ci][:], dtype=np.uint16) for ci, q in enumerate(qs)]
        out.append(dict(coef_up=up, quants=qout, hsamp0=int(job.out_hsamp0), vsamp0=int(job.out_vsamp0)))
    return stop, out, workspace


def quantsmooth_(coefs, quants, flags: int, niter: int, *, hsamp=None, vsamp=None, colorspace=None,
                 image_size=None, workspace: Workspace | None = None) -> dict:
    """The reference's do_quantsmooth on `coefs` in place (see the module text).

    quants[ci]: 64 quantisers (natural order) or None (component without a table).  Returns a dict:
      stop       int32 device tensor of one element: the reference's return value (0 done, 1 stopped)
      coef_up    UPSAMPLE_UV: the two replacement chroma tensors (luma geometry), else None
      quants     the output quant tables (all ones where a table was given, as the reference leaves them)
      hsamp0, vsamp0   component 0's output sampling factors
      workspace  the Workspace used; pass it again (also inside a graph capture) for jobs of the same geometry
    coef_up, hsamp0 and vsamp0 describe the result when `stop` reads 0; when it reads 1 the reference drops the
    replacement chroma and component 0 keeps its sampling factors (coef_up's contents are then meaningless)."""
    import torch
    dev = _check_tensors(coefs, torch)
    qs = _check_quants(quants, len(coefs))
    job = _device_job(_hip(), coefs, qs, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace, image_size=image_size)
    stop, (out,), workspace = _enqueue([job], [qs], dev, flags, niter, workspace, "quantsmooth_", True)
    return dict(stop=stop, **out, workspace=workspace)


def quantsmooth_batch_(images, flags: int, niter: int, *, workspace: Workspace | None = None) -> dict:
    """quantsmooth_ on many images in one call (qs_hip_do_quantsmooth_device_batch): their planes share kernel launches,
    so a batch of small or medium images fills the GPU where one image does not.  Results are quantsmooth_'s, image by
    image, bit for bit.

    images[i]: a dict with quantsmooth_'s per-image arguments -- coefs, quants and optionally hsamp, vsamp, colorspace,
    image_size.  One flags / niter setting for the whole batch.  All tensors on one device, none of them twice.
    Returns a dict:
      stop       int32 device tensor of len(images) elements: stop[i] is image i's return value (0 done, 1 stopped)
      images     per image: dict(coef_up, quants, hsamp0, vsamp0), as quantsmooth_ returns them
      workspace  the Workspace used; pass it again (also inside a graph capture) for a batch of the same geometry"""
    import torch
    who = "quantsmooth_batch_"
    hip = _hip()
    seen, jobs, tables = set(), [], []

    def one(i, im, _res):
        coefs = im["coefs"]
        if isinstance(coefs, (list, tuple)) and coefs:      # (the tables first: they need no device)
            qs = _check_quants(im["quants"], len(coefs), who=f"{who}: image {i}")
        d = _check_tensors(coefs, torch, who=f"{who}: image {i}")
        for t in coefs:
            if t.data_ptr() in seen:
                raise ValueError(f"{who}: image {i} passes a tensor (or its storage) that appears earlier in the batch")
            seen.add(t.data_ptr())
        tables.append(qs)
        jobs.append(_device_job(hip, coefs, qs, hsamp=im.get("hsamp"), vsamp=im.get("vsamp"),
                                colorspace=im.get("colorspace"), image_size=im.get("image_size")))
        return d

    dev, _stop = _images_on_one_device(images, None, who, ("coefs", "quants"), one, torch)
    stop, out, workspace = _enqueue(jobs, tables, dev, flags, niter, workspace, who, False)
    return dict(stop=stop, images=out, workspace=workspace)


# ---- decode to pixels (qs_hip_decode_device_batch) -------------------------------------------------------------------

def _decode_job(hip, coefs, quants, im, res, who, torch):
    """the qs_hip_job of one image to decode: its arrays and geometry, and what a smoothing result `res` reported
    (the output tables, UPSAMPLE_UV's replacement chroma)"""
    _check_tensors(coefs, torch, who=who)
    if res is not None:
        quants = res["quants"]
    qs = _check_quants(quants, len(coefs), who=who)
    up = res.get("coef_up") if res is not None else None
    if up is not None:
        _check_tensors(list(up), torch, who=f"{who}: coef_up")
    job = _device_job(hip, coefs, qs, hsamp=im.get("hsamp"), vsamp=im.get("vsamp"), colorspace=im.get("colorspace"),
                      image_size=im.get("image_size"), coef_up=None if up is None else (up[0].data_ptr(), up[1].data_ptr()))
    if up is not None:
        job.up_hblk, job.up_wblk = int(up[0].shape[0]), int(up[0].shape[1])
    return job


def _upsampling(value, who):
    from .hipqs import UPSAMPLING
    if not isinstance(value, str) or value not in UPSAMPLING:
        raise ValueError(f"{who}: upsampling {value!r}: \"dct\" (libjpeg 7..9, DCT-scaled chroma) or \"triangle\" "
                         f"(libjpeg-turbo / 6b, triangle-filter chroma upsampling)")
    return value


def _scale_denom(value, who):
    if isinstance(value, bool) or not isinstance(value, int) or value not in (1, 2, 4, 8):
        raise ValueError(f"{who}: scale_denom {value!r}: 1, 2, 4 or 8 (libjpeg 9's scale_num / scale_denom = 1 / N)")
    return value


def _decode_enqueue(jobs, dev, stop, outs, workspace, who, modes=None, scales=None):
    """the decode's workspace (prepared outside any capture when the geometry, tables, modes or scales changed), the
    outputs, the run.  modes: None (the calls without opts) or one "dct" / "triangle" per job; scales: None (full size)
    or one scale_denom per job"""
    import torch
    hip = _hip()
    per, total = hip.decode_batch_info(jobs, modes, scales)
    key = ("decode",) + tuple(_key(job, 0, 0) for job in jobs) + (() if modes is None else ("upsampling", tuple(modes))) \
        + (() if scales is None else ("scale_denom", tuple(scales)))
    workspace = _prepared(workspace, key, total, dev,
                          lambda ptr, nbytes, stream: hip.decode_batch_prepare(jobs, ptr, nbytes, stream, modes, scales),
                          who, "on the same geometry (workspace=...)")
    if outs is None:
        outs = [None] * len(jobs)
    res = []
    for i, (inf, o) in enumerate(zip(per, outs)):
        shape = (inf["height"], inf["width"], inf["channels"])
        if o is None:
            o = torch.empty(shape, dtype=torch.uint8, device=dev)
        elif not isinstance(o, torch.Tensor) or o.dtype != torch.uint8 or o.device != dev or tuple(o.shape) != shape:
            raise ValueError(f"{who}: output {i} must be a uint8 tensor of shape {shape} on {dev}")
        elif o.stride(2) != 1 or o.stride(1) != inf["channels"]:
            raise ValueError(f"{who}: output {i} must have contiguous rows (stride {o.stride()})")
        res.append(o)
    pitches = [int(o.stride(0)) if o.shape[0] > 1 else o.shape[1] * o.shape[2] for o in res]
    d_stop = None if stop is None else stop.data_ptr()
    hip.decode_batch(jobs, d_stop, [o.data_ptr() for o in res], pitches, workspace.buf.data_ptr(), workspace.nbytes,
                     torch.cuda.current_stream(dev).cuda_stream)
    return res, workspace


def _check_stop(stop, n, dev, who, torch):
    if not isinstance(stop, torch.Tensor) or stop.dtype != torch.int32 or stop.device != dev or stop.numel() != n \
            or not stop.is_contiguous():
        raise ValueError(f"{who}: result['stop'] must be the int32 device tensor of {n} element(s) the smoothing returned")


def decode(coefs, quants=None, *, hsamp=None, vsamp=None, colorspace=None, image_size=None, result=None, out=None,
           workspace: Workspace | None = None, upsampling="dct", scale_denom=1):
    """Decode coefficient tensors to pixels on the current stream, exactly as libjpeg 9 does (JDCT_ISLOW, its default
    upsampling -- 2x chroma by DCT scaling -- and default output colour space).  Returns a uint8 CUDA tensor
    (image_height, image_width, C): C = 1 for grayscale, 3 (RGB) for YCbCr and RGB images.

    upsampling="dct": libjpeg 7..9's DCT-scaled chroma.  upsampling="triangle": the pixels of libjpeg-turbo and
    libjpeg 6b (what Pillow, OpenCV and torchvision decode with) -- the 8x8 IDCT at chroma resolution, then jdsample.c's
    triangle filters, and turbo's colour tables (its green is one lower than libjpeg 9's on a few (Cb, Cr) pairs).
    Grayscale and RGB-kept images without subsampling come out the same in both.  Anything else raises ValueError.

    scale_denom=2, 4 or 8: what libjpeg 9 hands out with scale_num / scale_denom = 1 / N -- an image of
    ceil(width * M / 8) x ceil(height * M / 8) samples, M = 8 / N, from IDCTs of reduced size that read only the block's
    top-left coefficients (no full-size decode, no second pass).  Only with upsampling="dct"; any other value, or
    "triangle" with a reduced size, raises ValueError.

    coefs, quants, hsamp, vsamp, colorspace: as quantsmooth_ takes them; image_size = (width, height) is required.
    result: what quantsmooth_ returned for these coefs -- its output tables and replacement chroma are used, and for
    UPSAMPLE_UV the choice between the replacement chroma (stop 0) and the original chroma (stop 1) is made on the device
    from result['stop'], with no host synchronisation.  out: a preallocated uint8 tensor of that shape (rows may be
    padded).  workspace: a Workspace, prepared in place when the geometry or tables change (outside a capture) and
    reused as it is inside one: pass the same object to the call that is captured."""
    r = decode_batch([dict(coefs=coefs, quants=quants, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace,
                           image_size=image_size)],
                     result=_batch_result(result), outs=_outs_of(out), workspace=workspace, upsampling=upsampling,
                     scale_denom=scale_denom, _who="decode")
    return r["images"][0]


def decode_batch(images, *, result=None, outs=None, workspace: Workspace | None = None, upsampling="dct",
                 scale_denom=1, _who="decode_batch") -> dict:
    """decode on many images in one call (one kernel launch for up to 44 images).  images[i]: a dict with decode's
    per-image arguments (coefs, quants, hsamp, vsamp, colorspace, image_size, and optionally upsampling, which overrides
    this call's upsampling= for that image: one batch may mix modes).  result: what quantsmooth_batch_ returned
    for these images, in the same order.  outs: optional preallocated outputs.  Returns dict(images=[uint8 tensors],
    workspace=Workspace).  A change of mode prepares the workspace again (outside a capture), as a change of geometry
    does.  scale_denom: one value for every image or a list with one per image, and the key "scale_denom" of an image's
    dict overrides it: one batch may mix 1, 2, 4 and 8.  outs[i] has the scaled shape, and a change of scales prepares
    the workspace again as a change of mode does."""
    import torch
    who = _who
    _upsampling(upsampling, who)
    _check_list(images, who)
    modes = [upsampling if not isinstance(im, dict) or im.get("upsampling") is None
             else _upsampling(im["upsampling"], f"{who}: image {i}") for i, im in enumerate(images)]
    if isinstance(scale_denom, (list, tuple)):
        if len(scale_denom) != len(images):
            raise ValueError(f"{who}: scale_denom has {len(scale_denom)} entries for {len(images)} images")
        per_image = list(scale_denom)
    else:
        per_image = [scale_denom] * len(images)
    scales = [_scale_denom(d if not isinstance(im, dict) or im.get("scale_denom") is None else im["scale_denom"],
                           f"{who}: image {i}") for i, (im, d) in enumerate(zip(images, per_image))]
    for i, (m, d) in enumerate(zip(modes, scales)):
        if m == "triangle" and d != 1:
            raise ValueError(f"{who}: image {i}: upsampling \"triangle\" decodes at full size only (scale_denom {d}): at "
                             f"reduced sizes libjpeg-turbo runs other IDCTs, which this decode does not carry")
    if all(m == "dct" for m in modes):
        modes = None                                                    # (the calls without opts)
    if all(d == 1 for d in scales):
        scales = None                                                   # (the calls of the full-size decode)
    for i, im in enumerate(images):
        if isinstance(im, dict) and im.get("image_size") is None:
            raise ValueError(f"{who}: image {i} has no image_size: the decode needs (width, height)")
    if outs is not None and len(outs) != len(images):
        raise ValueError(f"{who}: one output (or None) per image")
    jobs, dev, stop = _encode_jobs(images, result, who, torch, needs_quants=True)
    px, workspace = _decode_enqueue(jobs, dev, stop, outs, workspace, who, modes, scales)
    return dict(images=px, workspace=workspace)


# ---- entropy coding to JPEG bytes (qs_hip_encode_device_batch) ----------------------------------------------------------

def _huff_tables(hip, huffman, n, who):
    """huffman: None, one dict(dc={index: (bits, huffval)}, ac={...}) for every image, or a list of such dicts / None"""
    if huffman is None:
        return None, b""
    per = huffman if isinstance(huffman, (list, tuple)) else [huffman] * n
    if len(per) != n:
        raise ValueError(f"{who}: one huffman entry (or None) per image")
    tabs = [None if h is None else hip.huff_tables(h.get("dc"), h.get("ac")) for h in per]
    return tabs, b"|".join(b"" if t is None else bytes(t) for t in tabs)


def _encode_jobs(images, result, who, torch, needs_quants=False):
    """the qs_hip_jobs of images that hold coefs, their device, and the smoothing result's stop tensor (or None).
    needs_quants (decode_batch): an image without a smoothing result must bring its tables; the scan coder needs none"""
    hip = _hip()
    jobs = []

    def one(i, im, res):
        if im.get("image_size") is None:
            raise ValueError(f"{who}: image {i} has no image_size: the encoder needs (width, height)")
        if needs_quants and res is None and im.get("quants") is None:
            raise ValueError(f"{who}: image {i} needs quants (or a smoothing result)")
        d = _check_tensors(im["coefs"], torch, who=f"{who}: image {i}")
        quants = im.get("quants") if im.get("quants") is not None else [None] * len(im["coefs"])
        jobs.append(_decode_job(hip, im["coefs"], quants, im, res, f"{who}: image {i}", torch))
        return d

    dev, stop = _images_on_one_device(images, result, who, ("coefs",), one, torch)
    return jobs, dev, stop


def _restart_opts(restart_interval, restart_in_rows, n, who):
    """the restart keywords of the encode calls -> None (neither given: the calls without options), or one
    (restart_interval, restart_in_rows) per image"""
    if restart_interval is None and restart_in_rows is None:
        return None
    cols = []
    for name, v in (("restart_interval", restart_interval), ("restart_in_rows", restart_in_rows)):
        if v is None:
            v = 0
        if hasattr(v, "tolist"):                                    # numpy arrays and tensors, of one value or of many
            v = v.tolist()
        vals = [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)] * n
        if len(vals) != n:
            raise ValueError(f"{who}: {name} must be an int or hold one per image")
        cols.append(vals)
    return list(zip(*cols))


def _block_shapes(w, h, hsamp, vsamp):
    """(hblk, wblk) of each component of a w x h image with these sampling factors: libjpeg's height_in_blocks and
    width_in_blocks, ceil(size * samp / (8 * max_samp))"""
    w, h, mh, mv = int(w), int(h), 8 * max(hsamp), 8 * max(vsamp)
    return [(-(-h * v // mv), -(-w * s // mh)) for s, v in zip(hsamp, vsamp)]


def _coef_outs(outs, i, shapes, dev, who, torch):
    """the coefficient tensors image i is written to: new ones of `shapes`, or the caller's outs[i], checked"""
    if outs is None or outs[i] is None:
        return [torch.empty((hb, wb, 64), dtype=torch.int16, device=dev) for hb, wb in shapes]
    coefs = list(outs[i])
    if len(coefs) != len(shapes) or _check_tensors(coefs, torch, who=f"{who}: output {i}") != dev:
        raise ValueError(f"{who}: output {i} must be {len(shapes)} tensors on {dev}")
    return coefs


def _mcu_geometry(hsamp, vsamp, image_size):
    """(MCUs per row, MCUs) of libjpeg's scan over these components: one block per MCU in a one-component scan"""
    w, h = image_size
    mh, mv = (1, 1) if len(hsamp) == 1 else (max(hsamp), max(vsamp))
    mx, my = -(-int(w) // (8 * mh)), -(-int(h) // (8 * mv))
    return mx, mx * my


def _scan_interval(opt, hsamp, vsamp, image_size):
    """the restart_interval libjpeg arrives at for a scan of this geometry (jcmaster.c): what DRI carries"""
    ri, rows = opt
    if rows > 0:
        return min(rows * _mcu_geometry(hsamp, vsamp, image_size)[0], 65535)
    return ri


def _encode_workspace(jobs, dev, tabs, tabkey, workspace, who, torch, opts=None):
    hip = _hip()
    per, total = hip.encode_batch_info(jobs, opts)
    key = ("encode", tabkey) + tuple(_key(job, 0, 0) for job in jobs) + (() if opts is None else ("restart", tuple(opts)))
    return per, _prepared(workspace, key, total, dev,
                          lambda ptr, nbytes, stream: hip.encode_batch_prepare(jobs, tabs, ptr, nbytes, stream, opts),
                          who, "on the same geometry and tables (workspace=...)")


def _encode_outs(outs, images, per, dev, default_bytes, who, torch):
    """the output buffers of an encode call: outs[i] as the caller gave it, checked, or a new one of
    default_bytes(i, per[i], the blocks of image i) bytes"""
    if outs is None:
        outs = [None] * len(images)
    if len(outs) != len(images):
        raise ValueError(f"{who}: one output (or None) per image")
    bufs = []
    for i, (inf, o, im) in enumerate(zip(per, outs, images)):
        if o is None:
            blocks = sum(int(t.shape[0]) * int(t.shape[1]) for t in im["coefs"])
            o = torch.empty(default_bytes(i, inf, blocks), dtype=torch.uint8, device=dev)
        elif not isinstance(o, torch.Tensor) or o.dtype != torch.uint8 or o.device != dev or o.dim() != 1 \
                or not o.is_contiguous() or o.numel() < 1:
            raise ValueError(f"{who}: output {i} must be a contiguous one-dimensional uint8 tensor on {dev}")
        bufs.append(o)
    return bufs


def _len_status(n, dev, torch):
    """the `len` and `status` tensors of an encode call"""
    return torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)


def _image_variants(images, result, who):
    """per image its geometry variants as [(hsamp, vsamp)], its quants and its colour space: variant 0 is what the device
    codes when stop reads 0 (the replacement chroma at 1x1 when the smoothing made one), variant 1 the original sampling"""
    out = []
    for i, im in enumerate(images):
        res = None if result is None else result["images"][i]
        ncomp = len(im["coefs"])
        hs, vs = list(im.get("hsamp") or [1] * ncomp), list(im.get("vsamp") or [1] * ncomp)
        quants = res["quants"] if res is not None else im.get("quants")
        if quants is None:
            raise ValueError(f"{who}: image {i} needs quants (or a smoothing result)")
        cs = im.get("colorspace") if im.get("colorspace") is not None else (3 if ncomp == 3 else 1)
        variants = [(hs, vs)]
        if res is not None and res.get("coef_up") is not None:
            variants = [([int(res.get("hsamp0") or 1)] + [1] * (ncomp - 1), [int(res.get("vsamp0") or 1)] + [1] * (ncomp - 1)),
                        (hs, vs)]
        out.append((variants, quants, cs))
    return out


def _marker_blob(hip, parts, dev, torch):
    """parts[i][v] = the marker byte strings of image i's variant v -- (head, mid), or (head,) alone -- in one device buffer
    -> (the buffer, one EncodeFrame per image, per image the bytes of its longest variant)"""
    blob, at = bytearray(), []
    for variants in parts:
        at.append([])
        for strings in variants:
            at[-1].append([])
            for s in strings:
                at[-1][-1].append((len(blob), len(s)))
                blob += s
    buf = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
    base = buf.data_ptr()
    frames = []
    for variants in at:
        v = variants + [None] * (2 - len(variants))
        frames.append(hip.encode_frame(*[[None if e is None else (base + e[k][0], e[k][1]) for e in v]
                                         for k in range(len(variants[0]))]))
    return buf, frames, [max(sum(nb for _at, nb in e) for e in variants) for variants in at]


def encode_scan_batch(images, *, result=None, huffman=None, outs=None, workspace: Workspace | None = None,
                      restart_interval=None, restart_in_rows=None) -> dict:
    """The entropy-coded segment of each image's baseline scan, exactly the bytes libjpeg 9 writes between the SOS header
    and EOI for jpeg_write_coefficients on these arrays, on the current stream and without host synchronisation.

    images[i]: decode_batch's per-image dict (coefs, hsamp, vsamp, colorspace, image_size; quants are not needed).
    result: what quantsmooth_batch_ returned (the replacement chroma is coded when its stop reads 0, the original
    arrays when it reads 1, chosen on the device).  huffman: None (the standard tables), or a dict(dc={0: (bits[17],
    huffval), ...}, ac={...}) for all images, or a list with one such dict or None per image.  outs: preallocated
    contiguous uint8 buffers (their size is the capacity); by default 32 bytes per block.  workspace: as decode_batch.
    restart_interval / restart_in_rows: libjpeg's fields of these names, an int for all images or one per image -- RSTn
    markers every restart_interval MCUs (0 .. 65535, 0: none), or every restart_in_rows MCU rows of the geometry the
    scan has, which wins when > 0; DC prediction starts again behind each marker.  None for both: the call without
    options (the same bytes as 0).
    Returns dict(segments=[uint8 tensors], len=int64 tensor, status=int32 tensor, workspace): segment i is
    segments[i][:len[i]] when status[i] is 0; status 2: the buffer holds less than len[i] bytes (retry with that
    size); 1: a coefficient out of libjpeg's range; 3: a symbol without a code in `huffman`; 4: the workspace was prepared
    with a restart interval at another address than it runs at (len is 0 for these three)."""
    return _encode_scan_batch(images, result, huffman, outs, workspace, "encode_scan_batch",
                              _restart_opts(restart_interval, restart_in_rows, len(images), "encode_scan_batch"))


def _encode_scan_batch(images, result, huffman, outs, workspace, who, opts=None):
    import torch
    jobs, dev, stop = _encode_jobs(images, result, who, torch)
    hip = _hip()
    tabs, tabkey = _huff_tables(hip, huffman, len(jobs), who)
    per, workspace = _encode_workspace(jobs, dev, tabs, tabkey, workspace, who, torch, opts)
    bufs = _encode_outs(outs, images, per, dev, lambda i, inf, blocks: min(
        inf["max_segment_bytes"], 4096 + (32 if opts is None else 36) * blocks), who, torch)
    length, status = _len_status(len(jobs), dev, torch)
    hip.encode_batch(jobs, None if stop is None else stop.data_ptr(), [o.data_ptr() for o in bufs],
                     [int(o.numel()) for o in bufs], length.data_ptr(), status.data_ptr(), workspace.buf.data_ptr(),
                     workspace.nbytes, torch.cuda.current_stream(dev).cuda_stream)
    return dict(segments=bufs, len=length, status=status, workspace=workspace)


def encode_scan(coefs, *, hsamp=None, vsamp=None, colorspace=None, image_size=None, result=None, huffman=None, out=None,
                workspace: Workspace | None = None, restart_interval=None, restart_in_rows=None) -> dict:
    """encode_scan_batch on one image -> dict(segment, len, status, workspace); len and status are device tensors of
    one element"""
    r = _encode_scan_batch([dict(coefs=coefs, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace, image_size=image_size)],
                           _batch_result(result), huffman, _outs_of(out), workspace, "encode_scan",
                           _restart_opts(restart_interval, restart_in_rows, 1, "encode_scan"))
    return dict(segment=r["segments"][0], len=r["len"], status=r["status"], workspace=r["workspace"])


def encode_histogram_batch(images, *, result=None, workspace: Workspace | None = None, restart_interval=None,
                           restart_in_rows=None) -> dict:
    """The symbol counts of each image's scan (qs_hip_encode_device_batch_histogram) -> dict(counts: int32 tensor
    (len(images), 4, 257) in the order DC 0, DC 1, AC 0, AC 1 -- entry 256 is libjpeg's reserved symbol and reads 1 --,
    status: int32 tensor, 1 where a coefficient is out of range; workspace).  restart_interval / restart_in_rows as
    encode_scan_batch: the DC differences are those of the restart scan.  No host synchronisation."""
    import torch
    who = "encode_histogram_batch"
    jobs, dev, stop = _encode_jobs(images, result, who, torch)
    opts = _restart_opts(restart_interval, restart_in_rows, len(jobs), who)
    _per, workspace = _encode_workspace(jobs, dev, None, b"", workspace, who, torch, opts)
    counts = torch.empty((len(jobs), 4, 257), dtype=torch.int32, device=dev)
    status = torch.empty(len(jobs), dtype=torch.int32, device=dev)
    _hip().encode_batch_histogram(jobs, None if stop is None else stop.data_ptr(), counts.data_ptr(), status.data_ptr(),
                                  workspace.buf.data_ptr(), workspace.nbytes, torch.cuda.current_stream(dev).cuda_stream)
    return dict(counts=counts, status=status, workspace=workspace)


_STATUS_TEXT = {1: "DCT coefficient out of range", 3: "Missing Huffman code table entry",     # libjpeg's wording
                4: "the workspace holds a restart interval, but the run does not know it: prepare it at the address it runs at"}


def encode_batch(images, *, result=None, optimize=False, huffman=None, restart_interval=None, restart_in_rows=None) -> list:
    """Complete baseline JPEG files (bytes) of the images, byte for byte what libjpeg 9 writes for jpeg_write_coefficients
    on a fresh compress object with these arrays, tables and sampling factors (jpeg_file.compose has the marker rules).

    images[i]: coefs, quants, hsamp, vsamp, colorspace, image_size; result: what quantsmooth_batch_ returned for them
    (its output tables, replacement chroma and stop decide what is written).  optimize: libjpeg's optimize_coding -- the
    histogram on the device, qs_hip_huff_optimal on the host.  huffman: caller tables instead (see encode_scan_batch).
    restart_interval / restart_in_rows: as encode_scan_batch; the file gets the DRI marker of the geometry written, and
    optimize counts the symbols of the restart scan.
    Reads len / status, which synchronises; a buffer that proved too small is retried once with the exact size.  Raises
    ValueError with libjpeg's message where libjpeg would stop over a coefficient or a missing code; with optimize, a
    table whose code lengths pass 32 (libjpeg's "Huffman code size table overflow") raises what HipQS.huff_optimal
    raises, QsHipError with QS_HIP_EINVAL -- encode_file_batch reports it as status 5."""
    import torch
    from . import jpeg_file
    who = "encode_batch"
    hip = _hip()
    n = len(images)
    opts = _restart_opts(restart_interval, restart_in_rows, n, who)
    stops = [0] * n if result is None else [int(v) for v in result["stop"].cpu().tolist()]
    # what each file's header describes: the smoothing's output tables and, for a standing UPSAMPLE_UV, 1x1 chroma
    desc = []
    for i, im in enumerate(images):
        res = None if result is None else result["images"][i]
        ncomp = len(im["coefs"])
        hs = list(im.get("hsamp") or [1] * ncomp)
        vs = list(im.get("vsamp") or [1] * ncomp)
        if res is not None and res.get("coef_up") is not None and stops[i] == 0:
            hs, vs = [int(res.get("hsamp0") or 1)] + [1] * (ncomp - 1), [int(res.get("vsamp0") or 1)] + [1] * (ncomp - 1)
        quants = res["quants"] if res is not None else im.get("quants")
        if quants is None:
            raise ValueError(f"{who}: image {i} needs quants (or a smoothing result)")
        cs = im.get("colorspace") if im.get("colorspace") is not None else (3 if ncomp == 3 else 1)
        desc.append(dict(quants=quants, hsamp=hs, vsamp=vs, colorspace=cs, image_size=tuple(im["image_size"]),
                         tbl=jpeg_file.table_assignment(cs, ncomp)))
    std = dict(dc={t: hip.huff_standard(0, t) for t in (0, 1)}, ac={t: hip.huff_standard(1, t) for t in (0, 1)})
    if optimize:
        if huffman is not None:
            raise ValueError(f"{who}: optimize and huffman exclude each other")
        h = encode_histogram_batch(images, result=result, restart_interval=restart_interval,
                                   restart_in_rows=restart_in_rows)
        bad = [i for i, s in enumerate(h["status"].cpu().tolist()) if s]
        if bad:
            raise ValueError(f"{who}: image {bad[0]}: {_STATUS_TEXT[1]}")
        counts = h["counts"].cpu().numpy()
        huffman = []
        for i, d in enumerate(desc):
            used = sorted(set(d["tbl"]))
            huffman.append(dict(dc={t: hip.huff_optimal(counts[i, t]) for t in used},
                                ac={t: hip.huff_optimal(counts[i, 2 + t]) for t in used}))
    per = huffman if isinstance(huffman, (list, tuple)) else [huffman] * n
    r = _encode_scan_batch(images, result, huffman, None, None, who, opts)
    lens, status = r["len"].cpu().tolist(), r["status"].cpu().tolist()
    if any(s == 2 for s in status):
        outs = [torch.empty(max(1, int(l)), dtype=torch.uint8, device=o.device) if s == 2 else o
                for o, l, s in zip(r["segments"], lens, status)]
        r = _encode_scan_batch(images, result, huffman, outs, r["workspace"], who, opts)
        lens, status = r["len"].cpu().tolist(), r["status"].cpu().tolist()
    files = []
    for i, (d, seg, l, s) in enumerate(zip(desc, r["segments"], lens, status)):
        if s:
            raise ValueError(f"{who}: image {i}: {_STATUS_TEXT.get(s, f'status {s}')}")
        h = per[i] or {}
        dc = {t: (h.get("dc") or {}).get(t, std["dc"][t]) for t in (0, 1)}
        ac = {t: (h.get("ac") or {}).get(t, std["ac"][t]) for t in (0, 1)}
        files.append(jpeg_file.compose(seg[:int(l)].cpu().numpy().tobytes(), d["quants"], d["hsamp"], d["vsamp"],
                                       d["colorspace"], d["image_size"], dc, ac,
                                       0 if opts is None else _scan_interval(opts[i], d["hsamp"], d["vsamp"], d["image_size"])))
    return files


def encode(coefs, quants=None, *, hsamp=None, vsamp=None, colorspace=None, image_size=None, result=None, optimize=False,
           huffman=None, restart_interval=None, restart_in_rows=None) -> bytes:
    """encode_batch on one image -> the JPEG file as bytes"""
    return encode_batch([dict(coefs=coefs, quants=quants, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace,
                              image_size=image_size)],
                        result=_batch_result(result), optimize=optimize,
                        huffman=huffman, restart_interval=restart_interval, restart_in_rows=restart_in_rows)[0]


# ---- optimal tables and whole files on the device (qs_hip_huff_optimal_device, qs_hip_encode_device_batch_files) ----------

TABLES_BYTES = 4 * 273 + 4       # sizeof(qs_hip_huff_tables): dc[2], ac[2] of bits[17] + huffval[256], has_dc[2], has_ac[2]


def huff_optimal_device(counts) -> dict:
    """The optimal Huffman tables of symbol counts, on the device and on the current stream (qs_hip_huff_optimal_device,
    one wave per table): counts = a contiguous int32 device tensor (..., 257) or (257,), entry 256 ignored -- what
    encode_histogram_batch returns.  -> dict(bits: uint8 (n, 17), huffval: uint8 (n, 256), status: int32 (n)) over the n
    tables in order; status 5: a code length above 32 (bits and huffval are then 0), where HipQS.huff_optimal raises.  No
    host synchronisation."""
    import torch
    who = "huff_optimal_device"
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int32 \
            or not counts.is_contiguous() or counts.dim() < 1 or counts.shape[-1] != 257 or counts.numel() < 257:
        raise ValueError(f"{who}: counts must be a contiguous int32 device tensor whose last dimension is 257")
    n = counts.numel() // 257
    dev = counts.device
    tables = torch.empty((n, 273), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _hip().huff_optimal_device(counts.data_ptr(), n, tables.data_ptr(), status.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream)
    return dict(bits=tables[:, :17], huffval=tables[:, 17:], status=status)


def huffman_of_tables(record) -> dict:
    """one row of encode_file_batch's `tables` (a qs_hip_huff_tables record, uint8[1096]) -> the dict(dc={index: (bits,
    huffval)}, ac={...}) encode_batch(huffman=...) takes; reads the tensor, which synchronises"""
    b = bytes(record.cpu().numpy().tobytes()) if hasattr(record, "cpu") else bytes(record)
    out = dict(dc={}, ac={})
    for w, (kind, t) in enumerate((("dc", 0), ("dc", 1), ("ac", 0), ("ac", 1))):
        if b[4 * 273 + w]:
            bits = list(b[w * 273:w * 273 + 17])
            out[kind][t] = (bits, list(b[w * 273 + 17:w * 273 + 17 + sum(bits)]))
    return out


def _file_frames(images, result, opts, optimize, huffman, who):
    """per image and geometry variant (_image_variants) the (head, mid) bytes of jpeg_file.compose_parts"""
    from . import jpeg_file
    hip = _hip()
    n = len(images)
    per = huffman if isinstance(huffman, (list, tuple)) else [huffman] * n
    std = None
    parts = []
    for i, (im, (variants, quants, cs)) in enumerate(zip(images, _image_variants(images, result, who))):
        size = tuple(im["image_size"])
        dc = ac = None
        if not optimize:
            if std is None:
                std = dict(dc={t: hip.huff_standard(0, t) for t in (0, 1)}, ac={t: hip.huff_standard(1, t) for t in (0, 1)})
            h = per[i] or {}
            dc = {t: (h.get("dc") or {}).get(t, std["dc"][t]) for t in (0, 1)}
            ac = {t: (h.get("ac") or {}).get(t, std["ac"][t]) for t in (0, 1)}
        parts.append([jpeg_file.compose_parts(quants, vh, vv, cs, size, dc, ac,
                                              0 if opts is None else _scan_interval(opts[i], vh, vv, size))
                      for vh, vv in variants])
    return parts


def _stage_files(workspace, key, parts, scratch_bytes, dev, torch):
    """workspace.files for `key`: the marker bytes `parts` (_marker_blob) and the scratch of a whole-file run in device
    memory.  A captured graph goes on pointing into both, so they live as long as the workspace"""
    buf, frames, fixed = _marker_blob(_hip(), parts, dev, torch)
    workspace.files = dict(key=key, buf=buf, frames=frames, fixed=fixed,
                           scratch=torch.empty(max(1, scratch_bytes), dtype=torch.uint8, device=dev))


def encode_file_batch(images, *, result=None, optimize=True, huffman=None, outs=None, workspace: Workspace | None = None,
                      restart_interval=None, restart_in_rows=None, scans=None, refinement=False) -> dict:
    """Complete baseline JPEG files in device memory, byte for byte what libjpeg 9 writes for jpeg_write_coefficients
    (encode_batch's files), on the current stream and without host synchronisation: qs_hip_encode_device_batch_files.

    images, result, huffman, restart_interval / restart_in_rows: as encode_batch (quants come from `result` when it is
    given).  optimize (the default): libjpeg's optimize_coding, with histogram, tables (Annex K.2, one wave per table)
    and DHT markers made on the device, so the tables follow the data also when a captured graph is replayed; it
    excludes huffman.  optimize=False: the standard tables, or the caller's.  outs: preallocated contiguous uint8 buffers
    (their size is the capacity).  workspace: as encode_scan_batch -- inside a graph capture it must come from an earlier
    call with the same images' geometry, tables, quants and options; it owns the frames' device bytes and the scratch, so
    keep it alive as long as a graph that was captured with it.
    For an image with two geometries (a smoothing result with replacement chroma) both variants' markers are composed --
    variant 1 with the original sampling factors and its own DRI value under restart_in_rows -- and the device takes the
    one its stop selects, for the head, the mid and the scan alike.
    Returns dict(files=[uint8 tensors], len=int64 tensor, status=int32 tensor, tables, workspace): file i is
    files[i][:len[i]] when status[i] is 0.  status as encode_scan_batch, plus 5: a table with a code length above 32
    (libjpeg's "Huffman code size table overflow").  tables: with optimize a uint8 tensor (len(images), 1096) of
    qs_hip_huff_tables records (huffman_of_tables reads one), else None.
    scans: None (the baseline file above), or a progressive scan script -- [(component indices, Ss, Se, Ah, Al)] as
    jpeg_file.spectral_script makes it, one for all images or a list of scripts, one per image -- for the PROGRESSIVE file
    libjpeg writes with cinfo.scan_info set (qs_hip_encode_progressive_device_batch_files): SOF2, every scan with its own
    optimal tables in front of it.  It requires optimize=True (libjpeg forces it) and every scan with Ah = 0; `tables` is
    then None.  The restart keywords count in each scan's own MCUs.
    refinement=True: scripts with successive-approximation refinement scans (Ah > 0) are written too, such as
    jpeg_file.simple_progression, the script of cjpeg -progressive."""
    if scans is not None:
        if not optimize or huffman is not None:
            raise ValueError("encode_file_batch: a scan script requires optimize=True and no huffman (progressive mode forces "
                             "optimal tables)")
        return _encode_progressive_batch(images, result, scans, outs, workspace, "encode_file_batch",
                                         _restart_opts(restart_interval, restart_in_rows, len(images), "encode_file_batch"),
                                         bool(refinement))
    return _encode_file_batch(images, result, optimize, huffman, outs, workspace, "encode_file_batch",
                              _restart_opts(restart_interval, restart_in_rows, len(images), "encode_file_batch"))


def _encode_progressive_batch(images, result, scans, outs, workspace, who, opts, refinement=False):
    import torch
    from . import jpeg_file
    jobs, dev, stop = _encode_jobs(images, result, who, torch)
    hip = _hip()
    n = len(jobs)
    scans = list(scans)
    if not scans:
        raise ValueError(f"{who}: an empty scan script")
    # a scan is (components, Ss, Se, Ah, Al): its second entry is a number, a script's second entry is a scan
    per_image = [scans] * n if len(scans[0]) == 5 and not isinstance(scans[0][1], (list, tuple)) else [list(s) for s in scans]
    if len(per_image) != n:
        raise ValueError(f"{who}: one scan script per image")
    for i, (script, im) in enumerate(zip(per_image, images)):
        if not jpeg_file.validate_script(script, len(im["coefs"])) and not refinement:
            raise ValueError(f"{who}: image {i}: the script holds refinement scans (Ah > 0), which are not implemented")
    popts = [hip.prog_opts(script, *(opts[i] if opts is not None else (0, 0)), refinement=refinement)
             for i, script in enumerate(per_image)]
    per, total, scratch_bytes = hip.encode_progressive_info(jobs, popts)
    heads = []                                                          # per image and geometry variant: SOI .. SOF2
    for im, (variants, quants, cs) in zip(images, _image_variants(images, result, who)):
        heads.append([jpeg_file.compose_parts(quants, vh, vv, cs, tuple(im["image_size"]), progressive=True)[0] for vh, vv in variants])
    key = ("progressive", refinement, tuple(tuple(map(tuple, s)) for s in per_image), tuple(opts or ()),
           tuple(_key(job, 0, 0) for job in jobs), tuple(tuple(h) for h in heads), str(dev))
    if workspace is None:
        workspace = Workspace()

    def prepare(ptr, nbytes, stream):
        hip.encode_progressive_prepare(jobs, popts, ptr, nbytes, stream)
        _stage_files(workspace, key, [[(head,) for head in variants] for variants in heads], scratch_bytes, dev, torch)

    workspace = _prepared(workspace, key, total, dev, prepare, who,
                          "with the same geometry, scripts and markers (workspace=...)")
    fs = workspace.files
    bufs = _encode_outs(outs, images, per, dev, lambda i, inf, blocks: fs["fixed"][i] + min(
        inf["max_body_bytes"], 4096 + 600 * inf["nscans"] + 40 * blocks), who, torch)
    length, status = _len_status(n, dev, torch)
    hip.encode_progressive_files(jobs, fs["frames"], None if stop is None else stop.data_ptr(), [o.data_ptr() for o in bufs],
                                 [int(o.numel()) for o in bufs], length.data_ptr(), status.data_ptr(), fs["scratch"].data_ptr(),
                                 int(fs["scratch"].numel()), workspace.buf.data_ptr(), workspace.nbytes,
                                 torch.cuda.current_stream(dev).cuda_stream)
    return dict(files=bufs, len=length, status=status, tables=None, workspace=workspace)


def _encode_file_batch(images, result, optimize, huffman, outs, workspace, who, opts):
    import torch
    if optimize and huffman is not None:
        raise ValueError(f"{who}: optimize and huffman exclude each other")
    jobs, dev, stop = _encode_jobs(images, result, who, torch)
    hip = _hip()
    n = len(jobs)
    tabs, tabkey = _huff_tables(hip, huffman, n, who)
    per, workspace = _encode_workspace(jobs, dev, tabs, tabkey, workspace, who, torch, opts)
    parts = _file_frames(images, result, opts, optimize, huffman, who)
    fkey = (bool(optimize), tuple(tuple(v) for v in parts), str(dev))
    if workspace.files is None or workspace.files["key"] != fkey:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: inside a graph capture the workspace must come from an earlier call with the same "
                               f"markers (workspace=...): uploading them copies from the host")
        _stage_files(workspace, fkey, parts, hip.encode_files_scratch_bytes(n), dev, torch)
    fs = workspace.files
    bufs = _encode_outs(outs, images, per, dev, lambda i, inf, blocks: fs["fixed"][i] + 4 * 277 + 2 + min(
        inf["max_segment_bytes"], 4096 + (32 if opts is None else 36) * blocks), who, torch)
    length, status = _len_status(n, dev, torch)
    tables = torch.empty((n, TABLES_BYTES), dtype=torch.uint8, device=dev) if optimize else None
    hip.encode_batch_files(jobs, fs["frames"], optimize, None if stop is None else stop.data_ptr(),
                           [o.data_ptr() for o in bufs], [int(o.numel()) for o in bufs], length.data_ptr(), status.data_ptr(),
                           None if tables is None else tables.data_ptr(), fs["scratch"].data_ptr(), int(fs["scratch"].numel()),
                           workspace.buf.data_ptr(), workspace.nbytes, torch.cuda.current_stream(dev).cuda_stream)
    return dict(files=bufs, len=length, status=status, tables=tables, workspace=workspace)


def encode_file(coefs, quants=None, *, hsamp=None, vsamp=None, colorspace=None, image_size=None, result=None, optimize=True,
                huffman=None, out=None, workspace: Workspace | None = None, restart_interval=None, restart_in_rows=None,
                scans=None, refinement=False) -> dict:
    """encode_file_batch on one image -> dict(file, len, status, tables, workspace); len and status are device tensors of
    one element"""
    if scans is not None:
        r = encode_file_batch([dict(coefs=coefs, quants=quants, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace,
                                    image_size=image_size)],
                              result=_batch_result(result), optimize=optimize, huffman=huffman, outs=_outs_of(out),
                              workspace=workspace,
                              restart_interval=restart_interval, restart_in_rows=restart_in_rows, scans=list(scans),
                              refinement=refinement)
        return dict(file=r["files"][0], len=r["len"], status=r["status"], tables=None, workspace=r["workspace"])
    r = _encode_file_batch([dict(coefs=coefs, quants=quants, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace,
                                 image_size=image_size)], _batch_result(result), optimize, huffman, _outs_of(out), workspace,
                           "encode_file", _restart_opts(restart_interval, restart_in_rows, 1, "encode_file"))
    return dict(file=r["files"][0], len=r["len"], status=r["status"], tables=r["tables"], workspace=r["workspace"])


# ---- reading a scan into coefficient tensors (qs_hip_read_device_batch) -----------------------------------------------------

_HEADER_BYTES = 1 << 16          # what read() copies to the host at first to find the SOS header (doubled while short)


def _read_header(data, torch, who):
    """the parsed markers (jpeg_file.parse) of a file given as bytes or as a uint8 tensor: only its first bytes are
    looked at, and only they are copied when the tensor is on the device"""
    from . import jpeg_file
    if isinstance(data, (bytes, bytearray, memoryview)):
        return jpeg_file.parse(bytes(data), header_only=True)
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise TypeError(f"{who}: a file is bytes or a contiguous one-dimensional uint8 tensor")
    n = _HEADER_BYTES
    while True:
        try:
            return jpeg_file.parse(data[:n].cpu().numpy().tobytes(), header_only=True)
        except ValueError:
            if n >= data.numel():
                raise
            n *= 2


def _huffman_of(p):
    """the file's tables as encode(huffman=...) takes them, when every component uses DC and AC table Td == Ta in {0, 1}"""
    if any(td != ta or td not in (0, 1) for td, ta in zip(p["dc_tbl"], p["ac_tbl"])):
        return None
    used = sorted(set(p["dc_tbl"]))
    return dict(dc={t: p["dc"][t] for t in used}, ac={t: p["ac"][t] for t in used})


def read_batch(datas, *, outs=None, workspace: Workspace | None = None, device=None, split=False) -> dict:
    """Read the scans of JPEG files into device coefficient tensors on the current stream: what libjpeg 9's
    jpeg_read_coefficients leaves in its arrays.  One lane reads one restart interval, so files with a small restart
    interval (this package's encode(restart_interval=...), jpegtran -restart) are the workload; a file without DRI is
    read by a single lane, and refused when it has more than 32 768 blocks.  Baseline or extended sequential Huffman,
    8 bits, one scan over all components (jpeg_file.parse raises ValueError for anything else).

    datas[i]: bytes, or a one-dimensional uint8 tensor on the host or the device.  Only the header -- the first bytes, up
    to the SOS marker -- is parsed on the host; bytes and host tensors are uploaded whole, device tensors are read where
    they lie.  outs[i]: preallocated contiguous int16 tensors (hblk, wblk, 64) per component, at least libjpeg's
    width_in_blocks x height_in_blocks (blocks outside the scan are zeroed).  workspace: as decode_batch; it also keeps
    the parsed headers: inside a graph capture nothing is copied to the host, the files must be device tensors and have
    the headers of the files the workspace was prepared with (the same sizes, tables and offsets; the scan bytes and
    what lies behind them may differ).  device: where to read when every file is on the host (default: the current one).
    Returns dict(images, status, workspace): images[i] is the dict quantsmooth_batch_, decode_batch and encode_batch take
    -- coefs, quants, hsamp, vsamp, colorspace, image_size -- with huffman (the file's tables in the form
    encode(huffman=...) takes, or None when a component's Td != Ta or a table id above 1 is used), restart_interval and
    status (a view of one element of `status`, the int32 tensor of the batch: 0 ok, 1 RSTn markers that do not match the
    interval, 2 an interval with too few or too many bytes, 3 bits without a code; the arrays are then unspecified).

    split=True takes the split route (qs_hip_read_split_device_batch): every restart interval -- the whole scan of a file
    without DRI -- is cut into segments of hipqs.READ_SPLIT_BYTES bytes, one lane decodes one segment, the segments find
    their entry states by self-synchronisation in hipqs.READ_SPLIT_ROUNDS launches and the DC predictions are rebuilt
    by a prefix sum.  There is no interval cap; the images and the capture rules are the same, the workspace is one of
    its own (a workspace prepared for one route is prepared again for the other), and status may also be 4: the
    segments did not synchronise, read the file with split=False.  The default stays False until the crossover
    between the routes is measured.

    A batch in which EVERY file's frame is progressive (SOF2) is handed to read_progressive_batch (split=True is then a
    ValueError); a batch that mixes progressive and sequential files raises ValueError naming the first file of the other
    kind.  Sequential files take exactly the path they took before that route existed."""
    return _read_batch(datas, outs, workspace, device, "read_batch", split)


def _read_batch(datas, outs, workspace, device, who, split=False):
    import torch
    _check_files(datas, outs, who)
    if torch.cuda.is_current_stream_capturing():
        headers = _stored_headers(datas, workspace, who, "header", torch)
        if headers[0].get("sof") == 0xC2:                               # a workspace of the progressive route
            if split:
                raise ValueError(f"{who}: split=True reads sequential files; these are progressive (SOF2)")
            return _read_progressive_batch(datas, outs, workspace, device, who)
        _check_file_types(datas, who, torch)
    else:
        # a sequential file takes the path below; a batch in which every frame is SOF2 goes to the progressive route
        headers, prog = [], []
        for i, d in enumerate(datas):
            try:
                headers.append(_read_header(d, torch, f"{who}: file {i}"))
                prog.append(False)
            except ValueError as e:
                if "(SOF2)" not in str(e):
                    raise
                headers.append(None)
                prog.append(True)
        if any(prog):
            if not all(prog):
                other = prog.index(not prog[0])
                raise ValueError(f"{who}: file 0 is {'progressive (SOF2)' if prog[0] else 'sequential'} and file {other} is "
                                 f"{'progressive (SOF2)' if prog[other] else 'sequential'}: a batch is read by one route")
            if split:
                raise ValueError(f"{who}: split=True reads sequential files; these are progressive (SOF2)")
            return _read_progressive_batch(datas, outs, workspace, device, who)
    hip = _hip()
    split = bool(split)

    def per_file(p):
        opt = hip.read_opts(p["dc"], p["ac"], p["dc_tbl"], p["ac_tbl"], p["restart_interval"])
        return opt, bytes(opt), p["scan_offset"], dict(huffman=_huffman_of(p), restart_interval=p["restart_interval"])

    return _read_files(datas, outs, workspace, device, who, headers, per_file,
                       "read-split" if split else "read", "on the same geometry and tables (workspace=...)",
                       partial(hip.read_batch_info, split=split), partial(hip.read_batch_prepare, split=split),
                       partial(hip.read_batch, split=split))


def _check_files(datas, outs, who):
    if not isinstance(datas, (list, tuple)) or not datas:
        raise ValueError(f"{who}: datas must be a non-empty list of files")
    if outs is not None and len(outs) != len(datas):
        raise ValueError(f"{who}: one output list (or None) per file")


def _check_file_types(datas, who, torch):
    for i, d in enumerate(datas):
        if isinstance(d, torch.Tensor):
            if d.dtype != torch.uint8 or d.dim() != 1 or not d.is_contiguous():
                raise TypeError(f"{who}: file {i} must be a contiguous one-dimensional uint8 tensor")
        elif not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError(f"{who}: a file is bytes or a contiguous one-dimensional uint8 tensor")


def _stored_headers(datas, workspace, who, parsed, torch, sof2=False):
    """inside a graph capture nothing is copied to the host: the headers the workspace was prepared with (sof2: with
    progressive files) stand for those of the files, which must lie on the device"""
    headers = getattr(workspace, "headers", None)
    if headers is None or len(headers) != len(datas) or (sof2 and headers[0].get("sof") != 0xC2):
        raise RuntimeError(f"{who}: inside a graph capture the workspace must come from an earlier call on files with "
                           f"the same headers (workspace=...): parsing a {parsed} copies it to the host")
    if not all(isinstance(d, torch.Tensor) and d.is_cuda for d in datas):
        raise RuntimeError(f"{who}: inside a graph capture the files must be device tensors")
    return headers


def _read_files(datas, outs, workspace, device, who, headers, per_file, tag, same, info, prepare, run):
    """what the readers share once the headers are there: the files onto the device, the coefficient outputs and the
    jobs over them, the workspace step, the run, the status tensor and its per-image views.  per_file(header) -> (the
    route's opts record of the file, the bytes of it that go into the key, the offset of the bytes the run is pointed
    at, the fields of the image dict that the route adds); tag and same: the key's tag and the words of _prepared; info, prepare, run: the route's HipQS calls"""
    import torch
    dev = next((d.device for d in datas if isinstance(d, torch.Tensor) and d.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    hip = _hip()
    bufs, at, jobs, opts, keyed, images = [], [], [], [], [], []
    for i, (d, p) in enumerate(zip(datas, headers)):
        if isinstance(d, torch.Tensor):
            if d.is_cuda and d.device != dev:
                raise ValueError(f"{who}: file {i} is on {d.device}, the batch on {dev}")
            buf = d if d.is_cuda else d.to(dev, non_blocking=True)
        else:
            buf = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
        opt, opt_key, offset, extra = per_file(p)
        if offset and buf.numel() <= offset:
            raise ValueError(f"{who}: file {i} ends with its SOS header")
        bufs.append(buf)
        at.append(offset)
        opts.append(opt)
        keyed.append(opt_key)
        w, h = p["image_size"]
        coefs = _coef_outs(outs, i, _block_shapes(w, h, p["hsamp"], p["vsamp"]), dev, who, torch)
        jobs.append(_device_job(hip, coefs, [None] * len(coefs), hsamp=p["hsamp"], vsamp=p["vsamp"],
                                colorspace=p["colorspace"] or 1, image_size=(w, h)))
        images.append(dict(coefs=coefs, quants=[q.copy() for q in p["quants"]], hsamp=list(p["hsamp"]),
                           vsamp=list(p["vsamp"]), colorspace=p["colorspace"], image_size=(w, h), **extra))
    _per, total = info(jobs, opts)
    key = (tag,) + tuple(_key(job, 0, 0) for job in jobs) + tuple(keyed)
    workspace = _prepared(workspace, key, total, dev,
                          lambda ptr, nbytes, stream: prepare(jobs, opts, ptr, nbytes, stream), who, same)
    workspace.headers = headers
    status = torch.empty(len(jobs), dtype=torch.int32, device=dev)
    run(jobs, [b.data_ptr() + a for b, a in zip(bufs, at)], [b.numel() - a for b, a in zip(bufs, at)], status.data_ptr(),
        workspace.buf.data_ptr(), workspace.nbytes, torch.cuda.current_stream(dev).cuda_stream)
    for i, im in enumerate(images):
        im["status"] = status[i:i + 1]
    return dict(images=images, status=status, workspace=workspace)


def read(data, *, out=None, workspace: Workspace | None = None, device=None, split=False) -> dict:
    """read_batch on one file -> its image dict (coefs, quants, hsamp, vsamp, colorspace, image_size, huffman,
    restart_interval, status) with the workspace used under `workspace`; split as read_batch takes it"""
    r = _read_batch([data], _outs_of(out), workspace, device, "read", split)
    return dict(r["images"][0], workspace=r["workspace"])


# ---- reading a progressive file into coefficient tensors (qs_hip_read_prog_device_batch) -----------------------------------

def read_progressive_batch(datas, *, outs=None, workspace: Workspace | None = None, device=None) -> dict:
    """Read PROGRESSIVE JPEG files (SOF2, Huffman, 8 bits: cjpeg -progressive, jpegtran -progressive, this package's
    encode_file(scans=...)) into device coefficient tensors on the current stream: what libjpeg 9's
    jpeg_read_coefficients leaves in its arrays.  One lane reads one restart interval of one scan, and scans that
    depend on each other -- a refinement on the scans it refines -- run in successive launches, one per level of the
    script (three for libjpeg's ten-scan script).  Files with restart intervals and batches are the workload; a file
    without DRI is read by one lane per scan, and refused when a scan has more than 32 768 blocks in an interval.

    datas, outs, workspace, device and the result are read_batch's.  The whole file is parsed on the host
    (jpeg_file.parse_progressive: markers only), so a device tensor is copied to the host once -- never inside a graph
    capture, where the workspace's stored headers are used: the files must then be device tensors with the header layout
    of the files the workspace was prepared with (the same tables, scans and offsets; a file whose scans start elsewhere
    ends with status 1).  images[i] holds read_batch's fields with huffman=None (the tables are per scan), scans (the
    script, as encode_file(scans=...) takes it) and restart_interval (the first scan's DRI value).  status: 0 ok; 1 the
    RSTn markers of a scan do not fit its interval, or a scan does not start at its prepared offset; 2 an interval with
    too few or too many bytes, or a file that stops inside a scan; 3 bits without a code, a run past the band's end or
    past the interval's blocks; the arrays are then unspecified."""
    return _read_progressive_batch(datas, outs, workspace, device, "read_progressive_batch")


def _read_progressive_batch(datas, outs, workspace, device, who):
    import torch
    from . import jpeg_file
    _check_files(datas, outs, who)
    _check_file_types(datas, who, torch)
    if torch.cuda.is_current_stream_capturing():
        headers = _stored_headers(datas, workspace, who, "file", torch, sof2=True)
    else:
        headers = [jpeg_file.parse_progressive(d.cpu().numpy().tobytes() if isinstance(d, torch.Tensor) else bytes(d))
                   for d in datas]
    hip = _hip()

    def per_file(p):
        opt = hip.read_prog_opts(p["scans"])                            # (a record that points to its scans: keyed by them)
        return opt, bytes(opt._scans), 0, dict(huffman=None, scans=list(p["script"]),
                                               restart_interval=p["scans"][0]["restart_interval"])

    return _read_files(datas, outs, workspace, device, who, headers, per_file,
                       "read-prog", "on the same geometry, scans and tables (workspace=...)",
                       hip.read_prog_batch_info, hip.read_prog_batch_prepare, hip.read_prog_batch)


def read_progressive(data, *, out=None, workspace: Workspace | None = None, device=None) -> dict:
    """read_progressive_batch on one file -> its image dict with the workspace used under `workspace`"""
    r = _read_progressive_batch([data], _outs_of(out), workspace, device, "read_progressive")
    return dict(r["images"][0], workspace=r["workspace"])


# ---- compressing pixels into coefficient tensors (qs_hip_compress_device_batch) ---------------------------------------------

def _compress_tables(im, n, who):
    """the image's tables: quants as given, or libjpeg's jpeg_set_quality(quality, TRUE) tables -- luminance for component
    0, chrominance for the others"""
    from . import synth
    quants, quality = im.get("quants"), im.get("quality")
    if (quants is None) == (quality is None):
        raise ValueError(f"{who}: give exactly one of quality and quants")
    if quants is None:
        if not 1 <= int(quality) <= 100:
            raise ValueError(f"{who}: quality {quality} is not in 1..100")
        return [synth.quality_table(synth.STD_LUMA if ci == 0 else synth.STD_CHROMA, int(quality)) for ci in range(n)]
    qs = _check_quants(quants, n, who=who)
    if any(q is None or q.min() < 1 for q in qs):
        raise ValueError(f"{who}: every component needs a table of 64 values in 1..65535")
    return [q.astype(np.uint16) for q in qs]


def compress(pixels, *, quality=None, quants=None, hsamp=None, vsamp=None, colorspace=None, fancy=False,
             downsampling="box", out=None, workspace: Workspace | None = None) -> dict:
    """Compress device pixels into quantised coefficient tensors on the current stream: exactly the arrays libjpeg 9
    holds after jpeg_write_scanlines with JDCT_ISLOW and smoothing_factor 0, i.e. what jpeg_read_coefficients returns
    for that file.  downsampling="box": do_fancy_downsampling = FALSE (box-filter chroma downsampling, the 8x8
    jpeg_fdct_islow for every component).  downsampling="dct": do_fancy_downsampling = TRUE, the default of libjpeg 9,
    cjpeg and jpeg_set_defaults (2x-subsampled chroma through jpeg_fdct_16x16 / _16x8 / _8x16 of the full-resolution
    samples; the h2v1 box first for 4x1) -- the inverse of decode's chroma upsampling.  Where chroma is not subsampled
    the two modes agree.  fancy=True still raises ValueError, as does any other downsampling.

    pixels: a uint8 CUDA tensor (H, W, 1) or (H, W, 3) with contiguous rows (any row pitch, any base alignment): gray,
    or RGB.  quality: libjpeg's jpeg_set_quality(q, TRUE) tables (luminance for component 0, chrominance for the
    others); or quants: one table of 64 values in 1..65535 (natural order) per component.  hsamp / vsamp: default 1x1;
    chroma must be 1x1 and luma 1x1, 2x1, 1x2, 2x2 or 4x1 (ValueError otherwise).  colorspace: 1 for one channel; 3
    (RGB -> YCbCr, the default) or 2 (RGB kept) for three.  out: preallocated contiguous int16 tensors (hblk, wblk, 64),
    at least libjpeg's width_in_blocks x height_in_blocks each; blocks outside that geometry are not written.
    workspace: as decode's -- a Workspace, prepared in place when the geometry or tables change (outside a capture) and
    reused as it is inside one.  Returns the image dict read returns, with exactly these keys -- coefs, quants, hsamp,
    vsamp, colorspace, image_size -- so quantsmooth_(**im, ...), decode(**im) and encode(**im, restart_interval=...)
    take it as it is."""
    r = compress_batch([dict(pixels=pixels, quality=quality, quants=quants, hsamp=hsamp, vsamp=vsamp,
                             colorspace=colorspace)], fancy=fancy, downsampling=downsampling,
                       outs=_outs_of(out),
                       workspace=workspace, _who="compress")
    return r["images"][0]


def _downsampling(value, who):
    from . import hipqs
    if not isinstance(value, str) or value not in hipqs.DOWNSAMPLING:
        raise ValueError(f"{who}: downsampling {value!r}: \"box\" (do_fancy_downsampling = FALSE) or \"dct\" (libjpeg 9's "
                         f"default, DCT-scaled chroma downsampling)")
    return value


def compress_batch(images, *, fancy=False, downsampling="box", outs=None, workspace: Workspace | None = None,
                   _who="compress_batch") -> dict:
    """compress on many images in one call (one kernel launch for up to 44 images).  images[i]: a dict with compress's
    per-image arguments (pixels, quality or quants, hsamp, vsamp, colorspace, and optionally downsampling, which
    overrides this call's downsampling= for that image: one batch may mix modes).  outs[i]: optional preallocated
    arrays.  Returns dict(images=[image dicts], workspace=Workspace)."""
    import torch
    who = _who
    _check_list(images, who)
    if fancy:
        raise ValueError(f"{who}: fancy=True is refused; libjpeg 9's default downsampling (2x chroma through 16-point "
                         f"scaled DCTs) is downsampling=\"dct\"")
    _downsampling(downsampling, who)
    if outs is not None and len(outs) != len(images):
        raise ValueError(f"{who}: one output list (or None) per image")
    hip = _hip()
    metas, modes = [], []

    def one(i, im, _res):
        w_i = f"{who}: image {i}"
        modes.append(downsampling if im.get("downsampling") is None else _downsampling(im["downsampling"], w_i))
        px = im["pixels"]
        if not isinstance(px, torch.Tensor) or px.dtype != torch.uint8 or not px.is_cuda:
            raise TypeError(f"{w_i}: pixels must be a uint8 CUDA (HIP) tensor")
        if px.dim() != 3 or px.shape[2] not in (1, 3) or px.shape[0] < 1 or px.shape[1] < 1:
            raise ValueError(f"{w_i}: pixels have shape {tuple(px.shape)}, expected (H, W, 1) or (H, W, 3)")
        n = int(px.shape[2])
        if px.stride(2) != 1 or px.stride(1) != n or (px.shape[0] > 1 and px.stride(0) < px.shape[1] * n):
            raise ValueError(f"{w_i}: pixels must have contiguous rows (stride {px.stride()})")
        cs = im.get("colorspace")
        cs = (1 if n == 1 else 3) if cs is None else int(cs)
        if (n == 1 and cs != 1) or (n == 3 and cs not in (2, 3)):
            raise ValueError(f"{w_i}: colour space {cs} for {n} channel(s): 1 (gray), or 3 (YCbCr) / 2 (RGB)")
        hs = [int(v) for v in (im.get("hsamp") or [1] * n)]
        vs = [int(v) for v in (im.get("vsamp") or [1] * n)]
        if len(hs) != n or len(vs) != n:
            raise ValueError(f"{w_i}: one sampling factor per component")
        if n == 3 and (hs[1:] != [1, 1] or vs[1:] != [1, 1] or (hs[0], vs[0]) not in ((1, 1), (2, 1), (1, 2), (2, 2), (4, 1))):
            raise ValueError(f"{w_i}: sampling {hs} x {vs}: chroma must be 1x1 and luma 1x1, 2x1, 1x2, 2x2 or 4x1")
        metas.append((px, n, cs, hs, vs, _compress_tables(im, n, w_i)))
        return px.device

    dev, _stop = _images_on_one_device(images, None, who, ("pixels",), one, torch)
    jobs, results = [], []
    for i, (px, n, cs, hs, vs, qs) in enumerate(metas):
        h, w = int(px.shape[0]), int(px.shape[1])
        coefs = _coef_outs(outs, i, _block_shapes(w, h, hs, vs), dev, who, torch)
        jobs.append(_device_job(hip, coefs, qs, hsamp=hs, vsamp=vs, colorspace=cs, image_size=(w, h)))
        results.append(dict(coefs=coefs, quants=[q.copy() for q in qs], hsamp=hs, vsamp=vs, colorspace=cs,
                            image_size=(w, h)))
    opts = modes if any(m != "box" for m in modes) else None      # (all box: the calls without opts)
    _per, total = hip.compress_batch_info(jobs, opts=opts)
    key = ("compress",) + tuple(_key(job, 0, 0) + (mode,) for job, mode in zip(jobs, modes))
    workspace = _prepared(workspace, key, total, dev,
                          lambda ptr, nbytes, stream: hip.compress_batch_prepare(jobs, ptr, nbytes, stream, opts=opts),
                          who, "on the same geometry and tables (workspace=...)")
    pitches = [int(m[0].stride(0)) if m[0].shape[0] > 1 else int(m[0].shape[1]) * m[1] for m in metas]
    hip.compress_batch(jobs, [m[0].data_ptr() for m in metas], pitches, workspace.buf.data_ptr(), workspace.nbytes,
                       torch.cuda.current_stream(dev).cuda_stream)
    return dict(images=results, workspace=workspace)
