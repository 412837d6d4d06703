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

torch is imported on first use only: importing the package does not need it."""
from __future__ import annotations

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
    stream = torch.cuda.current_stream(dev)
    if workspace is None or workspace.key != key:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: inside a graph capture the workspace must come from an earlier call of the same "
                               f"{'job' if single else 'batch'} (workspace=res['workspace']): preparing one synchronises")
        if workspace is None or workspace.nbytes < total or workspace.buf.device != dev:
            workspace = Workspace(torch.empty(max(1, total), dtype=torch.uint8, device=dev))
        prepare(arg, flags, niter, workspace.buf.data_ptr(), workspace.nbytes, stream.cuda_stream)
        workspace.key = key
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
    job = _hip().device_job([t.data_ptr() for t in coefs], [tuple(t.shape[:2]) for t in coefs], qs, hsamp=hsamp,
                            vsamp=vsamp, colorspace=colorspace, image_size=image_size)
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
    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError(f"{who}: images must be a non-empty list of dicts")
    dev, seen, jobs, tables = None, set(), [], []
    hip = _hip()
    for i, im in enumerate(images):
        if not isinstance(im, dict) or "coefs" not in im or "quants" not in im:
            raise ValueError(f"{who}: image {i} must be a dict with coefs and quants")
        coefs = im["coefs"]
        if isinstance(coefs, (list, tuple)) and coefs:      # (the tables first: they need no device)
            qs = _check_quants(im["quants"], len(coefs), who=f"{who}: image {i}")
        d = _check_tensors(coefs, torch, who=f"{who}: image {i}")
        if dev is None:
            dev = d
        elif d != dev:
            raise ValueError(f"{who}: image {i} is on {d}, image 0 on {dev}")
        for t in coefs:
            if t.data_ptr() in seen:
                raise ValueError(f"{who}: image {i} passes a tensor (or its storage) that appears earlier in the batch")
            seen.add(t.data_ptr())
        tables.append(qs)
        jobs.append(hip.device_job([t.data_ptr() for t in coefs], [tuple(t.shape[:2]) for t in coefs], qs,
                                   hsamp=im.get("hsamp"), vsamp=im.get("vsamp"), colorspace=im.get("colorspace"),
                                   image_size=im.get("image_size")))
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
    job = hip.device_job([t.data_ptr() for t in coefs], [tuple(t.shape[:2]) for t in coefs], qs, hsamp=im.get("hsamp"),
                         vsamp=im.get("vsamp"), colorspace=im.get("colorspace"), image_size=im.get("image_size"),
                         coef_up=None if up is None else (up[0].data_ptr(), up[1].data_ptr()))
    if up is not None:
        job.up_hblk, job.up_wblk = int(up[0].shape[0]), int(up[0].shape[1])
    return job


def _decode_enqueue(jobs, dev, stop, outs, workspace, who):
    """the decode's workspace (prepared outside any capture when the geometry or tables changed), the outputs, the run"""
    import torch
    hip = _hip()
    per, total = hip.decode_batch_info(jobs)
    key = ("decode",) + tuple(_key(job, 0, 0) for job in jobs)
    if workspace is None:
        workspace = Workspace()
    if workspace.key != key:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: inside a graph capture the workspace must come from an earlier call on the same "
                               f"geometry (workspace=...): preparing one synchronises")
        if workspace.nbytes < total or workspace.buf.device != dev:      # (filled in place: decode() returns no dict)
            workspace.buf = torch.empty(max(1, total), dtype=torch.uint8, device=dev)
        hip.decode_batch_prepare(jobs, workspace.buf.data_ptr(), workspace.nbytes, torch.cuda.current_stream(dev).cuda_stream)
        workspace.key = key
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
           workspace: Workspace | None = None):
    """Decode coefficient tensors to pixels on the current stream, exactly as libjpeg 9 does (JDCT_ISLOW, its default
    upsampling -- 2x chroma by DCT scaling -- and default output colour space).  Returns a uint8 CUDA tensor
    (image_height, image_width, C): C = 1 for grayscale, 3 (RGB) for YCbCr and RGB images.

    coefs, quants, hsamp, vsamp, colorspace: as quantsmooth_ takes them; image_size = (width, height) is required.
    result: what quantsmooth_ returned for these coefs -- its output tables and replacement chroma are used, and for
    UPSAMPLE_UV the choice between the replacement chroma (stop 0) and the original chroma (stop 1) is made on the device
    from result['stop'], with no host synchronisation.  out: a preallocated uint8 tensor of that shape (rows may be
    padded).  workspace: a Workspace, prepared in place when the geometry or tables change (outside a capture) and
    reused as it is inside one: pass the same object to the call that is captured."""
    r = decode_batch([dict(coefs=coefs, quants=quants, hsamp=hsamp, vsamp=vsamp, colorspace=colorspace,
                           image_size=image_size)],
                     result=None if result is None else dict(stop=result["stop"], images=[result]),
                     outs=None if out is None else [out], workspace=workspace, _who="decode")
    return r["images"][0]


def decode_batch(images, *, result=None, outs=None, workspace: Workspace | None = None, _who="decode_batch") -> dict:
    """decode on many images in one call (one kernel launch for up to 44 images).  images[i]: a dict with decode's
    per-image arguments (coefs, quants, hsamp, vsamp, colorspace, image_size).  result: what quantsmooth_batch_ returned
    for these images, in the same order.  outs: optional preallocated outputs.  Returns dict(images=[uint8 tensors],
    workspace=Workspace)."""
    import torch
    who = _who
    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError(f"{who}: images must be a non-empty list of dicts")
    for i, im in enumerate(images):
        if isinstance(im, dict) and im.get("image_size") is None:
            raise ValueError(f"{who}: image {i} has no image_size: the decode needs (width, height)")
    if result is not None and len(result["images"]) != len(images):
        raise ValueError(f"{who}: result holds {len(result['images'])} images, the batch {len(images)}")
    if outs is not None and len(outs) != len(images):
        raise ValueError(f"{who}: one output (or None) per image")
    hip = _hip()
    dev, jobs = None, []
    for i, im in enumerate(images):
        if not isinstance(im, dict) or "coefs" not in im:
            raise ValueError(f"{who}: image {i} must be a dict with coefs")
        res = None if result is None else result["images"][i]
        if res is None and im.get("quants") is None:
            raise ValueError(f"{who}: image {i} needs quants (or a smoothing result)")
        d = _check_tensors(im["coefs"], torch, who=f"{who}: image {i}")
        if dev is None:
            dev = d
        elif d != dev:
            raise ValueError(f"{who}: image {i} is on {d}, image 0 on {dev}")
        jobs.append(_decode_job(hip, im["coefs"], im.get("quants"), im, res, f"{who}: image {i}", torch))
    stop = None
    if result is not None:
        stop = result["stop"]
        _check_stop(stop, len(images), dev, who, torch)
    px, workspace = _decode_enqueue(jobs, dev, stop, outs, workspace, who)
    return dict(images=px, workspace=workspace)
