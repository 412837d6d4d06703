"""The scan geometry is one thing for the entropy coder and the scan reader: over a grid of frames, the coder's route
(qs_hip_encode_device_batch_info) and the reader's (qr_geometry of csrc/qs_read.h, compiled for the host:
tests/geom_host.cpp) accept and refuse the same frames and agree on the blocks of an MCU, the blocks of each component
and the blocks of the scan."""
import subprocess

from host_tools import build

SIZES = (1, 7, 8, 9, 16, 17, 65500)
MAXBITS = 27 + 63 * 26                                        # QS_ENC_MAXBITS: the longest code of one block


def _reader_grid(workdir):
    out = subprocess.run([str(build("geom_host.cpp"))], capture_output=True, text=True, check=True).stdout
    return [[int(x) for x in line.split()] for line in out.splitlines()]


def test_coder_and_reader_agree_on_every_frame_of_the_grid(pkg, hip, tmp_path):
    rows = _reader_grid(tmp_path)
    assert [tuple(r[:5]) for r in rows] == [(n, w, h, hs, vs) for n in (1, 3) for w in SIZES for h in SIZES
                                            for hs in range(1, 5) for vs in range(1, 5)]
    refused = set()
    for ncomp, W, H, h, v, rc, bpm, mcus, *blocks in rows:
        nw, nh = blocks[0::2][:ncomp], blocks[1::2][:ncomp]
        hs, vs = [h, 1, 1][:ncomp], [v, 1, 1][:ncomp]

        def coder(shapes):
            job = hip.device_job([0x100000 * (c + 1) for c in range(ncomp)], shapes, [None] * ncomp, hsamp=hs, vsamp=vs,
                                 colorspace=3 if ncomp == 3 else 1, image_size=(W, H))
            try:
                return 0, hip.encode_batch_info([job])[0][0]
            except pkg.hipqs.QsHipError as e:
                return e.code, None

        case = (ncomp, W, H, h, v)
        assert rc in (0, 2), case                             # (arrays large enough: only the 10-block limit refuses)
        if rc == 2:
            refused.add((ncomp, h, v))
            # the coder looks at the arrays first: give it libjpeg's own block counts, which the reader has filled in
        code, info = coder(list(zip(nh, nw)))
        assert code == (0 if rc == 0 else -4), case
        if rc:
            continue
        assert info["blocks_in_mcu"] == [bpm, bpm], case
        assert info["max_segment_bytes"] == 2 * ((mcus * bpm * MAXBITS + 7) // 8), case     # the blocks of the scan
        # the blocks of a component: the coder takes the reader's nw x nh and nothing narrower or shorter
        for c in range(ncomp):
            for dw, dh in ((1, 0), (0, 1)):
                if nw[c] - dw < 1 or nh[c] - dh < 1:
                    continue
                shapes = [(nh[k] - (dh if k == c else 0), nw[k] - (dw if k == c else 0)) for k in range(ncomp)]
                assert coder(shapes)[0] == -2, (case, c, dw, dh)
    # 3x3 + 2, 3x4 + 2, 4x3 + 2 and 4x4 + 2 blocks pass libjpeg's 10; one component is never interleaved
    assert refused == {(3, 3, 3), (3, 3, 4), (3, 4, 3), (3, 4, 4)}
