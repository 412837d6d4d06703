#!/usr/bin/env python3
"""Images per second of the device-resident route for a batch of full-HD 4:2:0 images, one stream (run on the MI355X).

For each quality it times, on the same device tensors:
  (a) loop     one torch_qs.quantsmooth_ call per image;
  (b) batch    one torch_qs.quantsmooth_batch_ call for all images;
  (c) graph    (b) captured into a torch.cuda.graph and replayed.
Each mode is warmed up, then timed with device events over windows of at least --window seconds, --repeats times, so
the spread shows.  The inputs are copied in before each call (the calls rewrite them in place); the copy is timed in
every mode alike.  (a) and (b) must leave identical bytes (coefficients, replacement chroma, stops): checked first.
Prints one JSON line.

--decode times the device decode to pixels instead (torch_qs.decode_batch, one launch per batch): 8192^2 grayscale,
8192^2 4:2:0 and --images x 1080p 4:2:0 in one batch, as time per call and GB/s of coefficients read plus samples
written; and, for 8192^2 4:2:0, the host alternative it replaces: the copy of the coefficients to the host plus
libjpeg 9's single-thread decode (tests/libjpeg9_decode.c, whose time includes writing the coefficients to an in-memory
JPEG first).  --upsampling triangle runs the same three cases in the decode's triangle mode (libjpeg-turbo's chroma
upsampling; no host alternative is timed).  --scale-denom 2|4|8 runs them at libjpeg 9's reduced sizes (DESIGN.md
section 12.2) and reports, per case, the full-size decode of the same arrays timed in the same session and the bytes
the scaled decode must move (the coefficients its IDCTs take -- exact, and as the 64-byte lines holding them -- plus
the samples out).

--encode times the device entropy coder (torch_qs.encode_scan_batch with the standard tables) on the same three cases:
the encode plus the device-to-host copy of `len` bytes, next to the host alternative it replaces -- the copy of the
coefficient arrays to the host (a lower bound of that route by itself) plus libjpeg 9's jpeg_write_coefficients on one
core (tests/libjpeg9_encode.c on a staged input file: its time includes reading the arrays and writing the file).
Medians of --repeats windows; exits non-zero unless the device route gives libjpeg's bytes and beats the copy alone.

--encode --optimize-files times the whole-file run with optimized tables instead (torch_qs.encode_file_batch: histogram,
table kernel, coder and framing in one call) on the same three cases with all-ones quant tables, in device time
(events around windows of calls, medians of --repeats): next to it the device work it replaces -- the histogram run plus
the plain run -- and, separately, the wall time of the route it replaces as a whole, torch_qs.encode_batch(optimize=True)
with its two host round trips; and the file sizes with the standard and with the optimized tables.  Exits non-zero
unless the first file of each case is libjpeg's optimized file.

--encode --progressive times the progressive run (torch_qs.encode_file_batch(scans=jpeg_file.spectral_script(n)): every
(job, scan) pair through histogram, table kernel, coder and framing) on the same three cases, in device time, next to the
baseline whole-file run with optimized tables on the same arrays in the same process, with the ratio of the two and the
sizes of the progressive and the baseline-optimized files.  Exits non-zero unless the first file of each case is the
file libjpeg writes with that script (tests/libjpeg9_encode.c).
--encode --progressive --script simple adds, per case, the run of jpeg_file.simple_progression (libjpeg's own script, four of
its ten YCbCr scans refinement scans) next to the spectral run and the baseline run on the same arrays, the file sizes, and
the time of the worst case of the refinement scans' run cutting (worst_case_last_bit_scan).

--read times the device scan reader (torch_qs.read_batch) on the same three cases, on files the device coder wrote with
--restart N / --restart-rows N: the upload of the file from pinned memory plus the read, and the read alone, next to the
host route it replaces -- libjpeg 9's jpeg_read_coefficients on one core (tests/libjpeg9_decode.c read: its time
includes writing the arrays to a file) plus the pinned upload of the coefficient arrays.  Parallelism is the number of
restart intervals: the lanes of each case are reported.  Exits non-zero unless the arrays are the ones encoded.
--read --split times the split route (read_batch(split=True): one lane per 256 bytes of an interval) and needs no
restart option; where the interval route accepts the same file its time on it is reported beside it
(interval_route_read_ms, null where it refuses the file), and both must give the arrays encoded.  --no-host leaves
libjpeg's read out.

--read --progressive [--script simple] times the progressive route of the scan reader (torch_qs.read_progressive_batch:
one lane per restart interval of one scan, one decode launch per level of the script) on the same three cases, on
progressive files the device progressive coder wrote with --restart N / --restart-rows N or without either (then one
lane reads each scan: the case the route is expected to lose): the upload of the file plus the read, and the read
alone, next to the host route on the same file -- libjpeg 9's jpeg_read_coefficients on one core plus the pinned upload
of the coefficient arrays.  A file the route refuses (an interval over the cap) is reported as refused; --batch-only --width 1280 --height 720
runs the batch case alone at a size the route reads without DRI.  Exits non-zero
unless the arrays read are the arrays encoded.

--compress times the device compress of pixels (torch_qs.compress_batch, one launch per batch, quality 50 tables) on the
same three cases, as time per call and GB/s of pixels read plus coefficients written, next to the decode of the arrays
it wrote (the same bytes the other way) and the host route it replaces: libjpeg 9's jpeg_write_scanlines on one core
(tests/libjpeg9_compress.c on a staged input file: its time includes reading the pixels and writing the file) plus the
pinned upload of the coefficient arrays.  Exits non-zero unless the arrays are libjpeg's.  --downsampling dct runs
the same three cases with libjpeg 9's default DCT-scaled chroma downsampling (do_fancy_downsampling = TRUE in the host
route and the comparison, tests/libjpeg9_compress_fancy.c) and reports whether each case's arrays coincide with the box
mode's: the gray case must.

    python tools/bench_device_batch.py [--images 32] [--qualities 3,6] [--niter 3] [--window 1.0] [--repeats 5]
                                       [--decode | --encode [--optimize-files | --progressive [--script simple]] | --read [--split | --progressive [--script simple]] [--no-host] | --compress]
                                       [--restart N | --restart-rows N]
                                       [--downsampling box|dct] [--upsampling dct|triangle] [--scale-denom 1|2|4|8]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--qualities", default="3,6")
    ap.add_argument("--niter", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--decode", action="store_true", help="time the device decode to pixels instead")
    ap.add_argument("--encode", action="store_true", help="time the device entropy coder instead")
    ap.add_argument("--restart", type=int, default=None, metavar="N",
                    help="--encode: write a restart marker every N MCUs (libjpeg's restart_interval)")
    ap.add_argument("--restart-rows", type=int, default=None, metavar="N",
                    help="--encode: write a restart marker every N MCU rows (libjpeg's restart_in_rows)")
    ap.add_argument("--optimize-files", action="store_true",
                    help="--encode: time the whole-file run with optimized tables next to the histogram run plus the plain run")
    ap.add_argument("--progressive", action="store_true",
                    help="--encode: time the progressive run (spectral selection) next to the baseline whole-file run")
    ap.add_argument("--script", choices=["spectral", "simple"], default="spectral",
                    help="--encode --progressive: simple also times jpeg_file.simple_progression (libjpeg's script, with "
                         "refinement scans) on the same arrays, and the worst case of its run cutting")
    ap.add_argument("--read", action="store_true", help="time the device scan reader instead (needs --restart / --restart-rows)")
    ap.add_argument("--split", action="store_true",
                    help="--read: the split route (segments of an interval in parallel); works without a restart option")
    ap.add_argument("--upsampling", choices=["dct", "triangle"], default="dct",
                    help="--decode: dct (libjpeg 9's DCT-scaled chroma) or triangle (libjpeg-turbo's triangle filters)")
    ap.add_argument("--scale-denom", type=int, choices=[1, 2, 4, 8], default=1,
                    help="--decode: libjpeg 9's reduced sizes (scale_num / scale_denom = 1 / N); the full-size decode of "
                         "the same arrays is timed in the same session, and the bytes the scaled decode must move are reported")
    ap.add_argument("--no-host", action="store_true", help="--read: do not time libjpeg's read of the file")
    ap.add_argument("--batch-only", action="store_true",
                    help="--read --progressive: only the batch of --images files of --width x --height (a size under the "
                         "interval cap shows the file without DRI: 1280 x 720)")
    ap.add_argument("--compress", action="store_true", help="time the device compress of pixels instead")
    ap.add_argument("--downsampling", choices=["box", "dct"], default="box",
                    help="--compress: box (do_fancy_downsampling = FALSE) or dct (libjpeg 9's default)")
    a = ap.parse_args()
    if a.compress:
        return bench_compress(a)
    if a.read and a.progressive:
        return bench_read_progressive(a)
    if a.read:
        return bench_read(a)
    if a.decode:
        return bench_decode(a)
    if a.encode and a.progressive:
        return bench_encode_progressive(a)
    if a.encode and a.optimize_files:
        return bench_encode_files(a)
    if a.encode:
        return bench_encode(a)

    import numpy as np
    import torch
    import jpegqs_pkg
    pkg = jpegqs_pkg.load()
    torch_qs = pkg.torch_qs
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nsrc = min(4, a.images)                                  # distinct inputs, repeated over the batch
    src = [pkg.synth.synth_ycc(a.width, a.height, 2, 2, quality=50, seed=11 + k) for k in range(nsrc)]
    pristine = [[torch.from_numpy(c).to(dev) for c in src[k % nsrc]["coefs"]] for k in range(a.images)]
    work = [[t.clone() for t in p] for p in pristine]
    kw = dict(hsamp=src[0]["hsamp"], vsamp=src[0]["vsamp"], colorspace=3, image_size=(a.width, a.height))
    quants = [src[k % nsrc]["quants"] for k in range(a.images)]
    blocks = sum(int(t.shape[0] * t.shape[1]) for t in pristine[0]) * a.images
    stream = torch.cuda.current_stream(dev)

    def reset():
        for w, p in zip(work, pristine):
            for t, s in zip(w, p):
                t.copy_(s)

    def timed(step, what):
        """images/s over windows of >= a.window s, a.repeats times (device events, after a warm-up)"""
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        per_call = max(time.perf_counter() - t0, 1e-6)
        calls = max(1, int(np.ceil(a.window / per_call)))
        rates = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                step()
            e1.record(stream)
            e1.synchronize()
            rates.append(calls * a.images / (e0.elapsed_time(e1) / 1e3))
        return dict(mode=what, calls_per_window=calls, images_per_s=[round(r, 1) for r in rates],
                    median_images_per_s=round(float(np.median(rates)), 1),
                    median_blocks_per_s=round(float(np.median(rates)) * blocks / a.images, 0))

    out = dict(tool="bench_device_batch", images=a.images, width=a.width, height=a.height, niter=a.niter,
               blocks_per_image=blocks // a.images, device=torch.cuda.get_device_name(dev), results=[])
    for quality in [int(q) for q in a.qualities.split(",")]:
        flags = pkg.flags_for_quality(quality)
        ws = {}

        def loop():
            reset()
            res = []
            for k, w in enumerate(work):
                r = torch_qs.quantsmooth_(w, quants[k], flags, a.niter, workspace=ws.get(k), **kw)
                ws[k] = r["workspace"]
                res.append(r)
            return res

        images = [dict(coefs=w, quants=quants[k], **kw) for k, w in enumerate(work)]
        bws = {}

        def batch():
            reset()
            r = torch_qs.quantsmooth_batch_(images, flags, a.niter, workspace=bws.get("ws"))
            bws["ws"] = r["workspace"]
            return r

        # identical bytes from (a) and (b)
        ra = loop()
        got_a = [[t.cpu() for t in w] for w in work] + [[t.cpu() for t in r["coef_up"]] for r in ra if r["coef_up"]]
        stop_a = [int(r["stop"].item()) for r in ra]
        rb = batch()
        got_b = [[t.cpu() for t in w] for w in work] + [[t.cpu() for t in r["coef_up"]] for r in rb["images"] if r["coef_up"]]
        stop_b = rb["stop"].cpu().tolist()
        same = stop_a == stop_b and len(got_a) == len(got_b) and all(
            torch.equal(x, y) for p, q in zip(got_a, got_b) for x, y in zip(p, q))
        if not same:
            raise SystemExit(f"bench_device_batch: quality {quality}: the loop and the batch differ")

        row = dict(quality=quality, flags=flags, identical_a_b=same, modes=[timed(loop, "a_loop"), timed(batch, "b_batch")])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            reset()
            torch_qs.quantsmooth_batch_(images, flags, a.niter, workspace=bws["ws"])
        row["modes"].append(timed(g.replay, "c_graph"))
        med = {m["mode"]: m["median_images_per_s"] for m in row["modes"]}
        row["b_over_a"] = round(med["b_batch"] / med["a_loop"], 2)
        row["c_over_a"] = round(med["c_graph"] / med["a_loop"], 2)
        out["results"].append(row)
        del g
    print(json.dumps(out), flush=True)


def bench_decode(a):
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from decode_oracle import LibJpeg9, synth_image
    torch_qs = jpegqs_pkg.load().torch_qs
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(1)
    cases = [("8192x8192_gray", [synth_image(rng, (8192, 8192), [1], [1], 1)]),
             ("8192x8192_420", [synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3)]),
             (f"{a.images}x1920x1080_420", [synth_image(rng, (1920, 1080), [2, 1, 1], [2, 1, 1], 3)] * a.images)]
    out = dict(tool="bench_device_batch", leg="decode", upsampling=a.upsampling, device=torch.cuda.get_device_name(dev),
               results=[])
    mode = dict(upsampling=a.upsampling) if a.upsampling != "dct" else {}      # (dct: the call as it always was)
    if a.scale_denom != 1:
        mode["scale_denom"] = a.scale_denom
        out["scale_denom"] = a.scale_denom

    def windows(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(20):
                call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / 20)
        return float(np.median(ms)), [round(m, 4) for m in ms]

    def scaled_traffic(im, outs_bytes):
        """what the scaled decode must move: the coefficients its IDCTs take (exact, and as the 64-byte lines that hold
        them: a block is two lines, rows 0..3 and 4..7) plus the samples out"""
        m = 8 // a.scale_denom
        hs, vs = (im["hsamp"][0], im["vsamp"][0]) if len(im["coefs"]) > 1 else (1, 1)
        exact = lines = 0
        for ci, c in enumerate(im["coefs"]):
            pw, ph = (m * min(hs, 2), m * vs) if ci else (m, m)
            nblk = c.shape[0] * c.shape[1]
            exact += nblk * pw * ph * 2
            lines += nblk * 64 * (2 if ph > 4 else 1)
        return exact + outs_bytes, lines + outs_bytes

    for name, ims in cases:
        images = [dict(coefs=[torch.from_numpy(c).to(dev) for c in im["coefs"]], quants=im["quants"], hsamp=im["hsamp"],
                       vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"]) for im in ims]
        ws = torch_qs.Workspace()
        outs = torch_qs.decode_batch(images, workspace=ws, **mode)["images"]
        nbytes = sum(sum(c.numel() * 2 for c in im["coefs"]) for im in images) + sum(o.numel() for o in outs)
        for _ in range(3):
            torch_qs.decode_batch(images, outs=outs, workspace=ws, **mode)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            calls = 20
            e0.record(stream)
            for _ in range(calls):
                torch_qs.decode_batch(images, outs=outs, workspace=ws, **mode)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / calls)
        med = float(np.median(ms))
        row = dict(case=name, images=len(images), mbytes=round(nbytes / 1e6, 1), ms=[round(m, 4) for m in ms],
                   median_ms=round(med, 4), gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1))
        if a.scale_denom != 1:
            exact = lines = 0
            for im, o in zip(images, outs):
                e, l = scaled_traffic(im, o.numel())
                exact += e
                lines += l
            fouts = torch_qs.decode_batch(images, workspace=torch_qs.Workspace())["images"]
            fws = torch_qs.Workspace()
            fmed, fms = windows(lambda: torch_qs.decode_batch(images, outs=fouts, workspace=fws))
            row.update(must_move_mbytes=round(exact / 1e6, 1), must_move_64B_lines_mbytes=round(lines / 1e6, 1),
                       gb_per_s_must_move=round(exact / (med * 1e-3) / 1e9, 1),
                       gb_per_s_64B_lines=round(lines / (med * 1e-3) / 1e9, 1),
                       full_size_ms=fms, full_size_median_ms=round(fmed, 4), full_over_scaled=round(fmed / med, 2))
            del fouts
        if name == "8192x8192_420" and a.upsampling == "dct" and a.scale_denom == 1:   # (libjpeg 9 is the host alternative of the dct mode)
            with tempfile.TemporaryDirectory() as td:
                lj9 = LibJpeg9(Path(td))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = [c.cpu().numpy() for c in images[0]["coefs"]]
                t1 = time.perf_counter()
                px = lj9.decode(host, ims[0]["quants"], ims[0]["hsamp"], ims[0]["vsamp"], 3, ims[0]["image_size"])
                t2 = time.perf_counter()
            row["host_alternative"] = dict(copy_ms=round((t1 - t0) * 1e3, 1), libjpeg9_ms=round((t2 - t1) * 1e3, 1),
                                           identical=bool(np.array_equal(px, outs[0].cpu().numpy())))
        out["results"].append(row)
    print(json.dumps(out), flush=True)


def host_writer(workdir, restart=None, restart_rows=None):
    """libjpeg 9 as the host side of --encode: (the helper that stages the input, write(staged) -> the file's bytes);
    with a restart option the helper that sets cinfo.restart_interval / restart_in_rows, so that the file compared and
    the write timed have the same markers as the device's segment"""
    sys.path.insert(0, str(ROOT / "tests"))
    if restart or restart_rows:
        from encode_rst_oracle import LibJpeg9EncRst
        enc = LibJpeg9EncRst(workdir)
        return enc, lambda staged: enc.run(staged, restart or 0, restart_rows or 0)
    from encode_oracle import LibJpeg9Enc
    enc = LibJpeg9Enc(workdir)
    return enc, enc.run


def bench_encode(a):
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from decode_oracle import synth_image
    from encode_oracle import parse_jpeg
    rst = dict(restart_interval=a.restart, restart_in_rows=a.restart_rows) if a.restart or a.restart_rows else {}
    if rst:
        from encode_rst_oracle import parse_rst
    torch_qs = jpegqs_pkg.load().torch_qs
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(1)
    cases = [("8192x8192_gray", [synth_image(rng, (8192, 8192), [1], [1], 1, amp=30)]),
             ("8192x8192_420", [synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3, amp=30)]),
             (f"{a.images}x1920x1080_420", [synth_image(rng, (1920, 1080), [2, 1, 1], [2, 1, 1], 3, amp=30)] * a.images)]
    out = dict(tool="bench_device_batch", leg="encode", device=torch.cuda.get_device_name(dev), results=[])
    if rst:
        out["restart"] = rst
    for name, ims in cases:
        images = [dict(coefs=[torch.from_numpy(c).to(dev) for c in im["coefs"]], hsamp=im["hsamp"], vsamp=im["vsamp"],
                       colorspace=im["colorspace"], image_size=im["image_size"]) for im in ims]
        ws = torch_qs.Workspace()
        r = torch_qs.encode_scan_batch(images, workspace=ws, **rst)
        outs, lens = r["segments"], [int(v) for v in r["len"].cpu().tolist()]
        assert r["status"].cpu().tolist() == [0] * len(images), "the default capacity did not hold the segment"
        pinned = [torch.empty(l, dtype=torch.uint8).pin_memory() for l in lens]
        coef_bytes = sum(sum(c.numel() * 2 for c in im["coefs"]) for im in images)

        def device_route():
            torch_qs.encode_scan_batch(images, outs=outs, workspace=ws, **rst)
            for p, o, l in zip(pinned, outs, lens):
                p.copy_(o[:l], non_blocking=True)
            torch.cuda.synchronize()

        def kernels_only():
            torch_qs.encode_scan_batch(images, outs=outs, workspace=ws, **rst)
            torch.cuda.synchronize()

        host_pinned = [[torch.empty(c.shape, dtype=torch.int16).pin_memory() for c in im["coefs"]] for im in images]

        def coef_copy():
            for hp, im in zip(host_pinned, images):
                for h, c in zip(hp, im["coefs"]):
                    h.copy_(c, non_blocking=True)
            torch.cuda.synchronize()

        def med(fn, calls):
            for _ in range(2):
                fn()
            ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                ms.append((time.perf_counter() - t0) * 1e3 / calls)
            return round(float(np.median(ms)), 3), [round(m, 3) for m in ms]

        dev_ms, dev_all = med(device_route, 10)
        k_ms, _ = med(kernels_only, 10)
        copy_ms, copy_all = med(coef_copy, 5)
        row = dict(case=name, images=len(images), coef_mbytes=round(coef_bytes / 1e6, 1), segment_bytes=sum(lens),
                   device_encode_plus_copy_ms=dev_ms, device_windows=dev_all, device_encode_ms=k_ms,
                   host_coef_copy_ms=copy_ms, host_copy_windows=copy_all, device_faster_than_copy=bool(dev_ms < copy_ms))
        with tempfile.TemporaryDirectory() as td:                   # the helper on a staged input: libjpeg reads the
            enc, write = host_writer(Path(td), a.restart, a.restart_rows)   # arrays, writes the file; one warm-up, then
            unit = [np.ones(64, np.uint16)] * len(ims[0]["coefs"])          # windows -- with the same restart interval
            staged = enc.stage(dict(ims[0], quants=unit))
            want = write(staged)
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                write(staged)
                ts.append((time.perf_counter() - t0) * 1e3)
            row["host_libjpeg9_write_ms_per_image"] = round(float(np.median(ts)), 1)
            row["host_libjpeg9_windows"] = [round(t, 1) for t in ts]
            seg = (parse_rst if rst else parse_jpeg)(want)["segment"]
            row["identical"] = all(seg == p.numpy().tobytes() for p, im in zip(pinned, ims) if im is ims[0])
        row["host_route_ms"] = round(copy_ms + row["host_libjpeg9_write_ms_per_image"] * len(images), 1)
        out["results"].append(row)
    print(json.dumps(out), flush=True)
    bad = [r["case"] for r in out["results"] if not (r["identical"] and r["device_faster_than_copy"])]
    if bad:                                                         # the bound of DESIGN.md section 13
        raise SystemExit(f"bench_device_batch --encode: {bad}: the device route must give libjpeg's bytes and be faster "
                         f"than the copy of the coefficient arrays alone")


def bench_encode_files(a):
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from decode_oracle import synth_image
    torch_qs = jpegqs_pkg.load().torch_qs
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rst = dict(restart_interval=a.restart, restart_in_rows=a.restart_rows) if a.restart or a.restart_rows else {}
    rng = np.random.default_rng(1)
    cases = [("8192x8192_gray", [synth_image(rng, (8192, 8192), [1], [1], 1, amp=30)]),
             ("8192x8192_420", [synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3, amp=30)]),
             (f"{a.images}x1920x1080_420", [synth_image(rng, (1920, 1080), [2, 1, 1], [2, 1, 1], 3, amp=30)] * a.images)]
    out = dict(tool="bench_device_batch", leg="encode --optimize-files", device=torch.cuda.get_device_name(dev), results=[])
    if rst:
        out["restart"] = rst
    for name, ims in cases:
        unit = [np.ones(64, np.uint16)] * len(ims[0]["coefs"])      # what the smoothing leaves: every quantiser 1
        images = [dict(coefs=[torch.from_numpy(c).to(dev) for c in im["coefs"]], quants=unit, hsamp=im["hsamp"],
                       vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"]) for im in ims]
        wf, wp = torch_qs.Workspace(), torch_qs.Workspace()
        r = torch_qs.encode_file_batch(images, workspace=wf, **rst)
        files, lens = r["files"], [int(v) for v in r["len"].cpu().tolist()]
        assert r["status"].cpu().tolist() == [0] * len(images), "the default capacity did not hold the file"
        s = torch_qs.encode_file_batch(images, optimize=False, workspace=torch_qs.Workspace(), **rst)
        std_lens = [int(v) for v in s["len"].cpu().tolist()]
        assert s["status"].cpu().tolist() == [0] * len(images)
        del s
        p = torch_qs.encode_scan_batch(images, workspace=wp, **rst)
        segs = p["segments"]

        def file_run():
            torch_qs.encode_file_batch(images, outs=files, workspace=wf, **rst)

        def replaced():
            torch_qs.encode_histogram_batch(images, workspace=wp, **rst)
            torch_qs.encode_scan_batch(images, outs=segs, workspace=wp, **rst)

        def histogram_only():
            torch_qs.encode_histogram_batch(images, workspace=wp, **rst)

        def med(fn, calls):
            for _ in range(2):
                fn()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / calls)
            return round(float(np.median(ms)), 3), [round(m, 3) for m in ms]

        f_ms, f_all = med(file_run, 10)
        r_ms, r_all = med(replaced, 10)
        h_ms, _ = med(histogram_only, 10)
        ts = []
        for _ in range(3):                                          # the route as a whole, with its host round trips
            t0 = time.perf_counter()
            host = torch_qs.encode_batch(images, optimize=True, **rst)
            ts.append((time.perf_counter() - t0) * 1e3)
        first = files[0][:lens[0]].cpu().numpy().tobytes()
        row = dict(case=name, images=len(images), file_run_ms=f_ms, file_run_windows=f_all, histogram_plus_plain_ms=r_ms,
                   histogram_plus_plain_windows=r_all, histogram_ms=h_ms, over_replaced=round(f_ms / r_ms, 4),
                   encode_batch_optimize_wall_ms=round(float(np.median(ts)), 1), standard_bytes=sum(std_lens),
                   optimized_bytes=sum(lens), optimized_over_standard=round(sum(lens) / sum(std_lens), 4),
                   identical_to_encode_batch=bool(host[0] == first))
        if rst:
            row["identical"] = row["identical_to_encode_batch"]      # (libjpeg's file with restarts: tests/test_gpu_encode_files.py)
        else:
            with tempfile.TemporaryDirectory() as td:
                from encode_oracle import LibJpeg9Enc
                enc = LibJpeg9Enc(Path(td))
                row["identical"] = bool(enc.write(dict(ims[0], quants=unit), optimize=True) == first)
        out["results"].append(row)
    print(json.dumps(out), flush=True)
    bad = [r["case"] for r in out["results"] if not r["identical"]]
    if bad:
        raise SystemExit(f"bench_device_batch --encode --optimize-files: {bad}: the file is not libjpeg's optimized file")


def bench_encode_progressive(a):
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from decode_oracle import synth_image
    pkg = jpegqs_pkg.load()
    torch_qs, jpeg_file = pkg.torch_qs, pkg.jpeg_file
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rst = dict(restart_interval=a.restart, restart_in_rows=a.restart_rows) if a.restart or a.restart_rows else {}
    rng = np.random.default_rng(1)
    cases = [("8192x8192_gray", [synth_image(rng, (8192, 8192), [1], [1], 1, amp=30)]),
             ("8192x8192_420", [synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3, amp=30)]),
             (f"{a.images}x1920x1080_420", [synth_image(rng, (1920, 1080), [2, 1, 1], [2, 1, 1], 3, amp=30)] * a.images)]
    out = dict(tool="bench_device_batch", leg="encode --progressive", device=torch.cuda.get_device_name(dev), results=[])
    if rst:
        out["restart"] = rst
    for name, ims in cases:
        unit = [np.ones(64, np.uint16)] * len(ims[0]["coefs"])
        images = [dict(coefs=[torch.from_numpy(c).to(dev) for c in im["coefs"]], quants=unit, hsamp=im["hsamp"],
                       vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"]) for im in ims]
        script = jpeg_file.spectral_script(len(ims[0]["coefs"]))
        wp, wf = torch_qs.Workspace(), torch_qs.Workspace()
        r = torch_qs.encode_file_batch(images, workspace=wp, scans=script, **rst)
        pfiles, plens = r["files"], [int(v) for v in r["len"].cpu().tolist()]
        assert r["status"].cpu().tolist() == [0] * len(images), "the default capacity did not hold the progressive file"
        b = torch_qs.encode_file_batch(images, workspace=wf, **rst)
        bfiles, blens = b["files"], [int(v) for v in b["len"].cpu().tolist()]
        assert b["status"].cpu().tolist() == [0] * len(images)

        def progressive_run():
            torch_qs.encode_file_batch(images, outs=pfiles, workspace=wp, scans=script, **rst)

        def baseline_run():
            torch_qs.encode_file_batch(images, outs=bfiles, workspace=wf, **rst)

        def med(fn, calls):
            for _ in range(2):
                fn()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / calls)
            return round(float(np.median(ms)), 3), [round(m, 3) for m in ms]

        b_ms, b_all = med(baseline_run, 10)
        p_ms, p_all = med(progressive_run, 10)
        b2_ms, b2_all = med(baseline_run, 10)                        # (again, behind the other: the pair's own spread)
        simple = None
        if a.script == "simple":
            # libjpeg's own script on the same arrays, in the same process; blocks read: the sum of the scans' blocks
            sscript = jpeg_file.simple_progression(len(ims[0]["coefs"]), ims[0]["colorspace"])
            wsim = torch_qs.Workspace()
            rs = torch_qs.encode_file_batch(images, workspace=wsim, scans=sscript, refinement=True, **rst)
            sfiles, slens = rs["files"], [int(v) for v in rs["len"].cpu().tolist()]
            assert rs["status"].cpu().tolist() == [0] * len(images), "the default capacity did not hold the simple_progression file"

            def simple_run():
                torch_qs.encode_file_batch(images, outs=sfiles, workspace=wsim, scans=sscript, refinement=True, **rst)

            s_ms, s_all = med(simple_run, 10)
            p2_ms, p2_all = med(progressive_run, 10)

            def blocks_read(sc):
                return sum(int(np.prod(ims[0]["coefs"][c].shape[:2])) for comps, *_r in sc for c in comps)
            simple = dict(scans=len(sscript), simple_ms=s_ms, simple_windows=s_all, spectral_again_ms=p2_ms,
                          spectral_again_windows=p2_all, simple_over_spectral=round(s_ms / min(p_ms, p2_ms), 3),
                          blocks_read_simple_over_spectral=round(blocks_read(sscript) / blocks_read(script), 3),
                          simple_bytes=sum(slens), simple_over_spectral_bytes=round(sum(slens) / sum(plens), 4),
                          simple_over_baseline_bytes=round(sum(slens) / sum(blens), 4))
            with tempfile.TemporaryDirectory() as td:
                from encode_prog_oracle import LibJpeg9EncProg
                simple["identical"] = bool(LibJpeg9EncProg(Path(td)).write(dict(ims[0], quants=unit), sscript, a.restart or 0,
                                                                           a.restart_rows or 0)
                                           == sfiles[0][:slens[0]].cpu().numpy().tobytes())
        first = pfiles[0][:plens[0]].cpu().numpy().tobytes()
        row = dict(case=name, images=len(images), scans=len(script), progressive_ms=p_ms, progressive_windows=p_all,
                   baseline_optimized_ms=b_ms, baseline_windows=b_all, baseline_again_ms=b2_ms, baseline_again_windows=b2_all,
                   progressive_over_baseline=round(p_ms / min(b_ms, b2_ms), 3), progressive_bytes=sum(plens),
                   baseline_optimized_bytes=sum(blens), progressive_over_baseline_bytes=round(sum(plens) / sum(blens), 4))
        with tempfile.TemporaryDirectory() as td:
            from encode_prog_oracle import LibJpeg9EncProg
            row["identical"] = bool(LibJpeg9EncProg(Path(td)).write(dict(ims[0], quants=unit), script, a.restart or 0,
                                                                    a.restart_rows or 0) == first)
        if simple is not None:
            row["simple_progression"] = simple
        out["results"].append(row)
    if a.script == "simple":
        out["worst_case_last_bit_scan"] = worst_case_refinement(a, torch, torch_qs, dev, med)
    print(json.dumps(out), flush=True)
    bad = [r["case"] for r in out["results"] if not r["identical"] or not r.get("simple_progression", {}).get("identical", True)]
    if bad:
        raise SystemExit(f"bench_device_batch --encode --progressive: {bad}: the file is not libjpeg's progressive file")


def worst_case_refinement(a, torch, torch_qs, dev, med):
    """8192 x 8192 gray with every AC coefficient +-2 or +-3: the last-bit scan of the band 1-63 writes no symbol of its
    own, every block leaves 63 correction bits, and the whole scan is one EOB run that is cut every 15 blocks -- the worst
    case of the run cutting.  The scan's time is the difference between the scripts with and without it; the AC scan that
    sends the band first is the ordinary scan of the same size next to it"""
    import numpy as np
    rng = np.random.default_rng(3)
    coef = (rng.integers(2, 4, (1024, 1024, 64)) * rng.choice([-1, 1], (1024, 1024, 64))).astype(np.int16)
    image = [dict(coefs=[torch.from_numpy(coef).to(dev)], quants=[np.ones(64, np.uint16)], hsamp=[1], vsamp=[1], colorspace=1,
                  image_size=(8192, 8192))]
    scripts = dict(dc=[((0,), 0, 0, 0, 0)], dc_ac=[((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)],
                   dc_ac_refine=[((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)])
    ms = {}
    for name, sc in scripts.items():
        ws = torch_qs.Workspace()
        r = torch_qs.encode_file_batch(image, workspace=ws, scans=sc, refinement=True)
        assert r["status"].cpu().tolist() == [0], name
        files = r["files"]

        def run():
            torch_qs.encode_file_batch(image, outs=files, workspace=ws, scans=sc, refinement=True)
        ms[name], _all = med(run, 10)
        ms[name + "_bytes"] = int(r["len"][0])
    return dict(case="8192x8192_gray_all_nonzero", ms=ms, ac_first_scan_ms=round(ms["dc_ac"] - ms["dc"], 3),
                last_bit_scan_ms=round(ms["dc_ac_refine"] - ms["dc_ac"], 3),
                last_bit_over_ac_first=round((ms["dc_ac_refine"] - ms["dc_ac"]) / (ms["dc_ac"] - ms["dc"]), 3))


def bench_read(a):
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from decode_oracle import LibJpeg9, synth_image
    if not (a.restart or a.restart_rows or a.split):
        raise SystemExit("bench_device_batch --read: give --restart N or --restart-rows N (one lane reads one interval), "
                         "or --split")
    rst = dict(restart_interval=a.restart, restart_in_rows=a.restart_rows) if a.restart or a.restart_rows else {}
    pkg = jpegqs_pkg.load()
    torch_qs = pkg.torch_qs
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(1)
    cases = [("8192x8192_gray", [synth_image(rng, (8192, 8192), [1], [1], 1, amp=30)]),
             ("8192x8192_420", [synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3, amp=30)]),
             (f"{a.images}x1920x1080_420", [synth_image(rng, (1920, 1080), [2, 1, 1], [2, 1, 1], 3, amp=30)] * a.images)]
    out = dict(tool="bench_device_batch", leg="read", device=torch.cuda.get_device_name(dev), restart=rst, results=[])
    if a.split:
        out.update(split=True, split_bytes=pkg.hipqs.READ_SPLIT_BYTES, split_rounds=pkg.hipqs.READ_SPLIT_ROUNDS)
    for name, ims in cases:
        im = ims[0]
        coefs = [torch.from_numpy(c).to(dev) for c in im["coefs"]]
        data = torch_qs.encode(coefs, im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                               image_size=im["image_size"], **rst)
        pinned = [torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory() for _ in ims]
        on_dev = [p.to(dev) for p in pinned]
        ws = torch_qs.Workspace()
        r = torch_qs.read_batch(on_dev, workspace=ws, split=a.split)
        outs = [x["coefs"] for x in r["images"]]
        status = r["status"].cpu().tolist()
        identical = status == [0] * len(ims) and all(torch.equal(g, c) for o in outs for g, c in zip(o, coefs))
        header = pkg.jpeg_file.parse(data, header_only=True)
        info_job = [pkg.HipQS.device_job([1] * len(coefs), [tuple(c.shape[:2]) for c in coefs], [None] * len(coefs),
                                         hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                                         image_size=im["image_size"])]
        info_opts = [pkg.HipQS.read_opts(header["dc"], header["ac"], header["dc_tbl"], header["ac_tbl"], header["restart_interval"])]
        per, _ = pkg.HipQS().read_batch_info(info_job, info_opts, split=a.split)

        def device_route():
            up = [p.to(dev, non_blocking=True) for p in pinned]
            torch_qs.read_batch(up, outs=outs, workspace=ws, split=a.split)
            torch.cuda.synchronize()

        def kernels_only():
            torch_qs.read_batch(on_dev, outs=outs, workspace=ws, split=a.split)
            torch.cuda.synchronize()

        host_pinned = [[torch.from_numpy(c).pin_memory() for c in im["coefs"]] for _ in ims]
        dst = [[torch.empty_like(c) for c in coefs] for _ in ims]

        def coef_upload():
            for hp, d in zip(host_pinned, dst):
                for h, t in zip(hp, d):
                    t.copy_(h, non_blocking=True)
            torch.cuda.synchronize()

        def med(fn, calls):
            for _ in range(2):
                fn()
            ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                ms.append((time.perf_counter() - t0) * 1e3 / calls)
            return round(float(np.median(ms)), 3), [round(m, 3) for m in ms]

        dev_ms, dev_all = med(device_route, 3)
        k_ms, k_all = med(kernels_only, 3)
        up_ms, _ = med(coef_upload, 3)
        row = dict(case=name, images=len(ims), file_bytes=len(data) * len(ims), coef_mbytes=round(sum(c.numel() * 2 for c in coefs) * len(ims) / 1e6, 1),
                   restart_interval=header["restart_interval"], lanes=per[0]["intervals"] * len(ims),
                   blocks_per_lane=per[0]["blocks_per_interval"], device_upload_plus_read_ms=dev_ms, device_windows=dev_all,
                   device_read_ms=k_ms, device_read_windows=k_all, host_coef_upload_ms=up_ms, identical=bool(identical))
        if a.split:                                                     # the interval route on the same file, where it takes it
            row.update(segments_at_most=per[0]["max_segments"] * len(ims), interval_route_read_ms=None)
            try:
                pkg.HipQS().read_batch_info(info_job, info_opts)
            except pkg.hipqs.QsHipError:
                pass                                                    # (over the interval cap)
            else:
                ws_old = torch_qs.Workspace()
                outs_old = [[torch.empty_like(c) for c in coefs] for _ in ims]

                def interval_route():
                    r = torch_qs.read_batch(on_dev, outs=outs_old, workspace=ws_old)
                    torch.cuda.synchronize()
                    return r
                ro = interval_route()
                same = ro["status"].cpu().tolist() == [0] * len(ims) and all(torch.equal(g, c) for o in outs_old for g, c in zip(o, coefs))
                row["identical"] = bool(identical and same)
                row["interval_route_read_ms"], row["interval_route_windows"] = med(interval_route, 1 if k_ms > 50 else 3)
                del ws_old, outs_old
        if a.no_host:
            out["results"].append(row)
            continue
        with tempfile.TemporaryDirectory() as td:
            lj9 = LibJpeg9(Path(td))
            f = Path(td) / "in.jpg"
            f.write_bytes(data)
            arrays = Path(td) / "out.bin"
            lj9._run("read", f, arrays)                                 # the helper alone: it writes the arrays to a file
            ts = []
            for _ in range(min(a.repeats, 3)):
                t0 = time.perf_counter()
                lj9._run("read", f, arrays)
                ts.append((time.perf_counter() - t0) * 1e3)
            row["host_libjpeg9_read_ms_per_image"] = round(float(np.median(ts)), 1)
        row["host_route_ms"] = round(up_ms + row["host_libjpeg9_read_ms_per_image"] * len(ims), 1)
        row["device_faster_than_host_route"] = bool(dev_ms < row["host_route_ms"])
        out["results"].append(row)
    print(json.dumps(out), flush=True)
    bad = [r["case"] for r in out["results"] if not r["identical"]]
    if bad:
        raise SystemExit(f"bench_device_batch --read: {bad}: the arrays read are not the arrays encoded")


def bench_read_progressive(a):
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from decode_oracle import LibJpeg9, synth_image
    rst = dict(restart_interval=a.restart, restart_in_rows=a.restart_rows) if a.restart or a.restart_rows else {}
    pkg = jpegqs_pkg.load()
    torch_qs, jpeg_file = pkg.torch_qs, pkg.jpeg_file
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(1)
    cases = [("8192x8192_gray", [synth_image(rng, (8192, 8192), [1], [1], 1, amp=30)]),
             ("8192x8192_420", [synth_image(rng, (8192, 8192), [2, 1, 1], [2, 1, 1], 3, amp=30)]),
             (f"{a.images}x{a.width}x{a.height}_420",
              [synth_image(rng, (a.width, a.height), [2, 1, 1], [2, 1, 1], 3, amp=30)] * a.images)]
    if a.batch_only:
        cases = cases[2:]
    out = dict(tool="bench_device_batch", leg="read_progressive", script=a.script, device=torch.cuda.get_device_name(dev),
               restart=rst, results=[])
    for name, ims in cases:
        im = ims[0]
        n = len(im["coefs"])
        script = jpeg_file.simple_progression(n, im["colorspace"]) if a.script == "simple" else jpeg_file.spectral_script(n)
        coefs = [torch.from_numpy(c).to(dev) for c in im["coefs"]]
        w = torch_qs.encode_file(coefs, im["quants"], hsamp=im["hsamp"], vsamp=im["vsamp"], colorspace=im["colorspace"],
                                 image_size=im["image_size"], scans=script, refinement=True, **rst)
        torch.cuda.synchronize()
        if int(w["status"][0]) != 0:
            raise SystemExit(f"bench_device_batch --read --progressive: {name}: the coder ended with status {int(w['status'][0])}")
        data = w["file"][:int(w["len"][0])].cpu().numpy().tobytes()
        del w
        header = jpeg_file.parse_progressive(data)
        row = dict(case=name, images=len(ims), file_bytes=len(data) * len(ims), scans=len(script),
                   coef_mbytes=round(sum(c.numel() * 2 for c in coefs) * len(ims) / 1e6, 1))
        info_job = [pkg.HipQS.device_job([1] * n, [tuple(c.shape[:2]) for c in coefs], [None] * n, hsamp=im["hsamp"],
                                         vsamp=im["vsamp"], colorspace=im["colorspace"], image_size=im["image_size"])]
        try:
            per, _ = pkg.HipQS().read_prog_batch_info(info_job, [pkg.HipQS.read_prog_opts(header["scans"])])
        except pkg.hipqs.QsHipError as e:
            row.update(refused=str(e), identical=True)
            out["results"].append(row)
            continue
        pinned = [torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory() for _ in ims]
        on_dev = [p.to(dev) for p in pinned]
        ws = torch_qs.Workspace()
        r = torch_qs.read_progressive_batch(on_dev, workspace=ws)
        outs = [x["coefs"] for x in r["images"]]
        status = r["status"].cpu().tolist()
        identical = status == [0] * len(ims) and all(torch.equal(g, c) for o in outs for g, c in zip(o, coefs))
        g = torch.cuda.CUDAGraph()                                      # the read alone: no host work per call
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            torch_qs.read_progressive_batch(on_dev, outs=outs, workspace=ws)

        def device_route():
            for p, d in zip(pinned, on_dev):
                d.copy_(p, non_blocking=True)
            g.replay()
            torch.cuda.synchronize()

        def kernels_only():
            g.replay()
            torch.cuda.synchronize()

        host_pinned = [[torch.from_numpy(c).pin_memory() for c in im["coefs"]] for _ in ims]
        dst = [[torch.empty_like(c) for c in coefs] for _ in ims]

        def coef_upload():
            for hp, d in zip(host_pinned, dst):
                for h, t in zip(hp, d):
                    t.copy_(h, non_blocking=True)
            torch.cuda.synchronize()

        def med(fn, calls):
            for _ in range(2):
                fn()
            ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                ms.append((time.perf_counter() - t0) * 1e3 / calls)
            return round(float(np.median(ms)), 3), [round(m, 3) for m in ms]

        k_ms, k_all = med(kernels_only, 1)
        dev_ms, dev_all = med(device_route, 1 if k_ms > 50 else 3)
        up_ms, _ = med(coef_upload, 3)
        row.update(levels=per[0]["levels"], lanes_per_scan=per[0]["intervals"], restart_interval=header["scans"][0]["restart_interval"],
                   device_upload_plus_read_ms=dev_ms, device_windows=dev_all, device_read_ms=k_ms, device_read_windows=k_all,
                   host_coef_upload_ms=up_ms, identical=bool(identical))
        del g
        if not a.no_host:
            with tempfile.TemporaryDirectory() as td:
                lj9 = LibJpeg9(Path(td))
                f = Path(td) / "in.jpg"
                f.write_bytes(data)
                arrays = Path(td) / "out.bin"
                lj9._run("read", f, arrays)                             # the helper alone: it writes the arrays to a file
                ts = []
                for _ in range(min(a.repeats, 3)):
                    t0 = time.perf_counter()
                    lj9._run("read", f, arrays)
                    ts.append((time.perf_counter() - t0) * 1e3)
                row["host_libjpeg9_read_ms_per_image"] = round(float(np.median(ts)), 1)
            row["host_route_ms"] = round(up_ms + row["host_libjpeg9_read_ms_per_image"] * len(ims), 1)
            row["device_over_host_route"] = round(dev_ms / row["host_route_ms"], 2)
        out["results"].append(row)
    print(json.dumps(out), flush=True)
    bad = [r["case"] for r in out["results"] if not r["identical"]]
    if bad:
        raise SystemExit(f"bench_device_batch --read --progressive: {bad}: the arrays read are not the arrays encoded")


def bench_compress(a):
    import subprocess
    import tempfile
    import numpy as np
    import torch
    import jpegqs_pkg
    sys.path.insert(0, str(ROOT / "tests"))
    from compress_oracle import Compress9, pack, tables
    mode = a.downsampling
    if mode == "dct":
        from compress_fancy_oracle import CompressFancy9 as Compress9   # libjpeg with do_fancy_downsampling = TRUE
    pkg = jpegqs_pkg.load()
    torch_qs, synth = pkg.torch_qs, pkg.synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_batch: no GPU visible (this tool measures the device only)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)

    def picture(w, h, n):
        return np.stack([synth.synth_pixels(w, h, 1234, variant=c) for c in range(n)], axis=-1)

    s420 = dict(hsamp=[2, 1, 1], vsamp=[2, 1, 1])
    cases = [("8192x8192_gray", picture(8192, 8192, 1), dict(hsamp=[1], vsamp=[1]), 1),
             ("8192x8192_420", picture(8192, 8192, 3), s420, 1),
             (f"{a.images}x1920x1080_420", picture(1920, 1080, 3), s420, a.images)]
    out = dict(tool="bench_device_batch", leg="compress", downsampling=mode, device=torch.cuda.get_device_name(dev),
               results=[])

    def windows(fn, calls=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / calls)
        return float(np.median(ms)), [round(m, 4) for m in ms]

    for name, px, samp, count in cases:
        n = px.shape[2]
        on_dev = [torch.from_numpy(px).to(dev) for _ in range(count)]
        images = [dict(pixels=t, quality=50, **samp) for t in on_dev]
        ws, dws = torch_qs.Workspace(), torch_qs.Workspace()
        kw = dict(downsampling=mode) if mode != "box" else {}
        res = torch_qs.compress_batch(images, workspace=ws, **kw)["images"]
        outs = [im["coefs"] for im in res]
        nbytes = sum(t.numel() for t in on_dev) + sum(c.numel() * 2 for o in outs for c in o)
        med, ms = windows(lambda: torch_qs.compress_batch(images, outs=outs, workspace=ws, **kw))
        back = torch_qs.decode_batch(res, workspace=dws)["images"]
        dmed, dms = windows(lambda: torch_qs.decode_batch(res, outs=back, workspace=dws))
        row = dict(case=name, images=count, mbytes=round(nbytes / 1e6, 1), ms=ms, median_ms=round(med, 4),
                   gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1), decode_ms=dms, decode_median_ms=round(dmed, 4),
                   compress_over_decode=round(med / dmed, 2))
        if mode != "box":                                  # the same pixels through the box mode: equal without subsampling
            box = torch_qs.compress_batch(images[:1])["images"][0]["coefs"]
            row["same_as_box"] = [bool(torch.equal(x, y)) for x, y in zip(box, outs[0])]
            del box
        # the host route: libjpeg 9 on one core, then the arrays up from pinned memory
        host_pinned = [[c.cpu().pin_memory() for c in o] for o in outs]
        dst = [[torch.empty_like(c) for c in o] for o in outs]

        def upload():
            for hp, d in zip(host_pinned, dst):
                for h, t in zip(hp, d):
                    t.copy_(h, non_blocking=True)
            torch.cuda.synchronize()

        for _ in range(2):
            upload()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            upload()
            ts.append((time.perf_counter() - t0) * 1e3)
        row["host_coef_upload_ms"] = round(float(np.median(ts)), 3)
        with tempfile.TemporaryDirectory() as td:
            c9 = Compress9(Path(td))
            q = tables("q50", n, synth)
            cs = 1 if n == 1 else 3
            staged, jpg = Path(td) / "in.bin", Path(td) / "out.jpg"
            staged.write_bytes(pack(px, q, samp["hsamp"], samp["vsamp"], cs))
            ts = []
            for _ in range(a.repeats + 1):                                 # (the first run warms the page cache)
                t0 = time.perf_counter()
                subprocess.run([str(c9.exe), "image", str(staged), str(jpg)], check=True)
                ts.append((time.perf_counter() - t0) * 1e3)
            row["host_libjpeg9_compress_ms_per_image"] = round(float(np.median(ts[1:])), 1)
            want = c9.lj9.read(jpg)["coefs"]
            row["identical"] = all(np.array_equal(w, c.cpu().numpy()) for o in outs for w, c in zip(want, o))
        row["host_route_ms"] = round(row["host_coef_upload_ms"] + row["host_libjpeg9_compress_ms_per_image"] * count, 1)
        out["results"].append(row)
        del on_dev, images, res, outs, back, host_pinned, dst
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    bad = [r["case"] for r in out["results"] if not r["identical"]]
    if bad:
        raise SystemExit(f"bench_device_batch --compress: {bad}: the arrays are not libjpeg's")
    if mode != "box" and not all(out["results"][0]["same_as_box"]):
        raise SystemExit("bench_device_batch --compress: the gray case does not coincide with the box mode")


if __name__ == "__main__":
    main()
