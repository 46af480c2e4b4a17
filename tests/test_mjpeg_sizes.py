"""CPU: the fixtures of tests/test_mjpeg_sizes_gpu.py reach the size-dependent
paths of the Motion-JPEG kernels they exist for. Every property is read from the
references alone (tests/mjpeg_ref.py for the encoder, Pillow's bytes for the
decoder), never from the kernels: 257 restart segments, a 64-block chunk of more
than 4096 bytes whose successor starts off a byte boundary, stuffed 0xFF bytes at
1080p, restart markers that straddle a chunk's and a scan window's end, batches
whose segment counts land in each `lanes` bucket with a remainder; and the
identity the 1080p encoder check rests on: a restart segment is the reference
encoder's output for its MCU row alone."""
import numpy as np
import pytest

from tests import mjpeg_cases as C
from tests import mjpeg_dec_cases as D
from tests import mjpeg_dec_ref as R

# jpegd_kernels.h kJpegdChunks: the workgroups (equal byte ranges) of a frame in k_jpegd_count / k_jpegd_index
CHUNKS = 32
# k_jpegd_index's threads: it walks its chunk in windows of this many bytes
WINDOW = 256
# jpeg_kernels.h kJpegChunk: the blocks k_jpeg_pack assembles in LDS at a time; it writes them out 1024 bytes a trip
PACK_BLOCKS, PACK_TRIP = 64, 1024

# (case, frames in the call): the decoder batches of tests/test_mjpeg_sizes_gpu.py -> (lanes, remainder)
LANE_BATCHES = {("pil136x104_gray_b1", 19): (2, 1), ("pil136x104_gray_b1_q95", 28): (3, 2),
                ("pil136x104_gray_b1", 149): (16, 1), ("pil136x104_b1", 67): (2, 1)}
# the variants of the gray batches in which a marker's 0xFF ends a chunk (a) / a window inside a chunk (b)
STRADDLE = {"pil136x104_gray_b1": {"a": 3, "b": 0}, "pil136x104_gray_b1_q95": {"a": 0, "b": 1}}
# (variant, MCU row): where the Python reference decoder is held equal to Pillow on the 1080p streams
HD_ROWS = [(0, 33), (0, 67), (1, 0), (1, 50)]


def huff_lanes(segs):
    """jpegd_launch (jpegd_kernels.hip): lanes = clamp(segs / kHuffWaves, 1, kHuffMaxLanes) = clamp(segs / 2048, 1, 16)."""
    return min(16, max(1, segs // 2048))


# ---- encoder -------------------------------------------------------------------------
@pytest.mark.parametrize("name,gray", [("rst_wrap32x160", False), ("noise70x37_q90", False), ("noise70x37_q90", True)])
def test_segment_reference_is_the_whole_frame_references_segment(name, gray):
    """Every segment of rst_wrap32x160, and noise70x37_q90 with its partial last strip (37 = 2 * 16 + 5
    = 4 * 8 + 5): the strip's own encode equals the whole frame's segment."""
    for v in (0, 1):
        segs, marks = C.split_stream(C.reference(name, v, gray)["stream"])
        assert len(segs) == -(-C.frame(name).shape[0] // (8 if gray else 16)) and marks[-1] == 0xD9
        for i, s in enumerate(segs):
            assert C.segment_reference(name, v, i, gray) == s, (name, v, i)
        assert sum(C.segment_stuffed(name, v, i, gray) for i in range(len(segs))) == C.reference(name, v, gray)["stuffed"]


@pytest.mark.parametrize("name", ["tall8x2056_gray", "tall16x4112"])
def test_tall_frames_have_257_segments(name):
    """k_jpeg_gather sums seglen 256 entries a trip: the 257th is the second trip's; RST0..7 wrap 32 times."""
    for v in (0, 1):
        segs, marks = C.split_stream(C.reference(name, v, C.SIZE_GRAY[name])["stream"])
        assert len(segs) == 257 and marks == [0xD0 + i % 8 for i in range(256)] + [0xD9]
        assert all(len(s) > 0 for s in segs)
    assert C.reference(name, 0, C.SIZE_GRAY[name])["stream"] != C.reference(name, 1, C.SIZE_GRAY[name])["stream"]


@pytest.mark.parametrize("name,nblocks", [("dense176x16_q100", 66), ("dense520x8_q100_gray", 65)])
def test_dense_segments_fill_a_chunk_and_carry_a_partial_byte(name, nblocks):
    """The reference gives, for variants 0 and 1: dense176x16_q100 4451 and 4453 bytes in the first 64
    blocks, the 65th at bit 4 and bit 7 of its byte; dense520x8_q100_gray 5402 and 5409 bytes, bits 3 and 1."""
    gray = C.SIZE_GRAY[name]
    for v in (0, 1):
        ref = C.reference(name, v, gray)
        off, total = C.block_bit_offsets(name, v, gray)
        assert len(off) == nblocks > PACK_BLOCKS and off == sorted(off)
        segs, _ = C.split_stream(ref["stream"])
        assert len(segs) == 1 and (total + 7) // 8 + ref["stuffed"] == len(segs[0])   # the offsets are this stream's
        first = off[PACK_BLOCKS] // 8                              # whole bytes the first chunk writes out
        assert first > 4 * PACK_TRIP, f"{name} variant {v}: {first} bytes"   # at least 5 trips of the 1024-byte loop
        assert off[PACK_BLOCKS] % 8 != 0                           # the second chunk takes a real partial byte
        assert total > off[PACK_BLOCKS] + 8


def test_hd_segments_hold_stuffed_bytes():
    """(the segments tests/test_mjpeg_sizes_gpu.py compares)"""
    H, W = C.frame(C.HD_CASE, 0).shape[:2]
    assert (W, H) == (1920, 1080) and not np.array_equal(C.frame(C.HD_CASE, 0), C.frame(C.HD_CASE, 1))
    for v, i in [(1, 0), (1, 67), (0, 67)]:
        s = C.segment_reference(C.HD_CASE, v, i)
        n = C.segment_stuffed(C.HD_CASE, v, i)
        assert n > 0 and s.count(b"\xff\x00") == n == s.count(b"\xff")


# ---- decoder -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", [n for n in D.SIZE_CASES if "1920" not in n])
def test_reference_decoder_equals_pillow_on_the_small_size_cases(name, variant):
    assert np.array_equal(D.expected("pil", name, None, variant), D.pillow_frame(name, variant))


def _data(name, v):
    j = D.stream("pil", name, None, v)
    return j[D.header_len(j):]


@pytest.mark.parametrize("name", list(STRADDLE))
def test_restart_markers_straddle_a_chunk_end_and_a_window_end(name):
    """(a) a marker's 0xFF is a chunk's last byte: its second byte is the next workgroup's;
    (b) it is the last byte of a 256-byte window inside a chunk: the second byte is the next trip's."""
    for cond, v in STRADDLE[name].items():
        d = _data(name, v)
        part = -(-len(d) // CHUNKS)
        assert part > WINDOW                                       # two windows a chunk
        marks = D.rst_offsets(d)
        assert len(marks) == 220 and len(marks) / CHUNKS > 6       # about 7 markers a chunk
        at_chunk_end = [p for p in marks if p % part == part - 1]
        at_window_end = [p for p in marks if p % part != part - 1 and (p % part) % WINDOW == WINDOW - 1]
        assert (at_chunk_end if cond == "a" else at_window_end), (name, cond, v)
    # markers in both windows of one chunk, after markers in earlier chunks
    d = _data(name, 0)
    part = -(-len(d) // CHUNKS)
    first = {p // part for p in D.rst_offsets(d) if p % part < WINDOW}
    second = {p // part for p in D.rst_offsets(d) if p % part >= WINDOW}
    assert (first & second) - {0}


def test_every_variant_of_a_batch_is_a_different_frame():
    for name in ("pil136x104_gray_b1", "pil136x104_gray_b1_q95", "pil136x104_b1"):
        n = max(k for (c, k) in LANE_BATCHES if c == name)
        streams = [D.stream("pil", name, None, v) for v in range(n)]
        hl = D.header_len(streams[0])
        assert len(set(streams)) == n and all(s[:hl] == streams[0][:hl] for s in streams)   # one header a batch


@pytest.mark.parametrize("name,n", list(LANE_BATCHES))
def test_decoder_batches_land_in_their_lane_buckets(name, n):
    h = R.parse(D.stream("pil", name, None, 0))
    m = 16 if len(h["comps"]) == 3 else 8
    mcus = -(-h["W"] // m) * -(-h["H"] // m)
    nseg = -(-mcus // h["dri"])
    assert nseg == (63 if len(h["comps"]) == 3 else 221)
    lanes, rem = LANE_BATCHES[(name, n)]
    assert huff_lanes(n * nseg) == lanes and (n * nseg) % lanes == rem != 0
    assert huff_lanes(8 * nseg) == huff_lanes(3 * nseg) == 1       # a handle of max_batch 8: 8 + 8 + 3 at one lane


def test_damaged_frames_of_the_shared_wave_batch():
    """Frame 13 keeps its 220 markers and runs out of data (one lane of k_jpegd_huff returns early),
    frame 20 has 219 (k_jpegd_index refuses it)."""
    case = ("pil", "pil136x104_gray_b1_q95", None)
    hdr, data = D.damaged("truncated", case, 28, 13, ((20, "no_rst"),))
    assert len(D.rst_offsets(data[13])) == 220 and len(D.rst_offsets(data[20])) == 219
    for f in (13, 20):
        with pytest.raises(R.Damaged):
            R.decode(hdr + data[f])
    assert data[12] == _data(case[1], 12) and np.array_equal(R.decode(hdr + data[14]), D.pillow_frame(case[1], 14))
    # with 3 lanes a wave, frames 13 and 20 share waves with their neighbours' segments
    assert huff_lanes(28 * 221) == 3 and (13 * 221) % 3 != 0 and (20 * 221) % 3 != 0


@pytest.mark.parametrize("variant,row", HD_ROWS)
def test_reference_decoder_equals_pillow_on_sampled_rows_at_1080p(variant, row):
    """The Python decoder is too slow for a whole 1080p frame. MCU row r of the frame depends on the
    segments of rows r - 1 .. r + 1 alone (chroma upsampling reaches one chroma row up and down), so the
    reference decodes a stream of those rows and is compared on row r."""
    name = "pil1920x1080_rows1"
    jpg = D.stream("pil", name, None, variant)
    h = R.parse(jpg)
    assert (h["W"], h["H"], h["dri"]) == (1920, 1080, 120) and len(D.rst_offsets(jpg[h["start"]:])) == 67
    assert (len(jpg) - h["start"]) // CHUNKS > 10000               # chunks of tens of windows
    lo, hi = max(row - 1, 0), min(row + 1, 67)
    sub = R.decode(D.mcu_rows_jpeg(jpg, lo, hi))
    got = sub[(row - lo) * 16:(row - lo) * 16 + 16]
    want = D.pillow_frame(name, variant)[16 * row:16 * row + 16]
    assert got.shape == want.shape and got.shape[0] == (8 if row == 67 else 16)
    assert np.array_equal(got, want)
