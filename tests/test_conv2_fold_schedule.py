"""CPU: the barrier protocol of the folded conv2 strip kernels (csrc/conv2_fwd_strip.h, csrc/conv2_dgrad_strip.h, FOLD = true) replayed in
plain Python.  A workgroup's run of strips becomes a sequence of intervals separated by workgroup barriers:

    P    stage(first strip)                                                        | barrier
    per strip, per tile t:
    [A]  MFMAs of t read the strip image; fold(pending) reads `red`;               | barrier B1
         data gradient, strip's last tile: stage(next strip) writes the OTHER image
    [W]  partials of t -> `red`; pending = t;                                      | barrier B2
         forward, strip's last tile: stage(next strip) writes the image
    F    fold(pending)

Every buffer access is tagged with the tile or strip it means.  Checked: no buffer is read and written inside one interval; every read
sees the version it means; every tile is folded exactly once with its own output base and valid count; every wave passes the same
number of barriers (the model has no wave-dependent control flow, and a workgroup without strips returns ahead of the first barrier)."""
import pytest

R = 2  # output rows (forward) / cell rows (data gradient) per strip


def forward_run(first, last, Ho, Wo):
    """Items first .. last - 1 of the forward kernel: strips of R output rows, tiles of 32 pixels; the last strip of an odd Ho is short."""
    strips_per_frame = (Ho + R - 1) // R
    ntiles = (R * Wo + 31) // 32
    run = []
    for item in range(first, last):
        img, k = divmod(item, strips_per_frame)
        ho0 = k * R
        npix = min(R, Ho - ho0) * Wo
        tiles = [dict(id=(item, t), outs=[dict(base=(img * Ho + ho0) * Wo * 64 + 32 * t * 64, valid=max(0, min(32, npix - 32 * t)))])
                 for t in range(ntiles)]
        run.append(dict(id=item, tiles=tiles))
    return run


def dgrad_run(first, last, H, W):
    """Items of the data-gradient kernel: strips of R cell rows, one tile per cell row, two output rows (row classes) per tile; a row
    below the image has no extent."""
    strips_per_frame = ((H + 1) // 2 + R - 1) // R
    run = []
    for item in range(first, last):
        img, k = divmod(item, strips_per_frame)
        tiles = []
        for t in range(R):
            h2 = k * R + t
            tiles.append(dict(id=(item, t), outs=[dict(base=((img * H + 2 * h2 + q) * W) * 32, valid=W * 32 if 2 * h2 + q < H else 0)
                                                  for q in range(2)]))
        run.append(dict(id=item, tiles=tiles))
    return run


def replay(kind, run):
    """-> (intervals, folds, barriers per wave).  An interval is a list of (buffer, 'r' | 'w', tag)."""
    barriers = [0] * 8
    if not run:  # the workgroup's early return, ahead of the first barrier
        return [], [], barriers
    intervals, folds = [], []

    def barrier():
        for w in range(8):
            barriers[w] += 1

    cur = 0
    image = (lambda c: f"img{c}") if kind == "dgrad" else (lambda c: "img")
    intervals.append([(image(cur), "w", run[0]["id"])])
    barrier()
    pending = None
    for i, strip in enumerate(run):
        nxt = run[i + 1] if i + 1 < len(run) else None
        for t, tile in enumerate(strip["tiles"]):
            last_tile = t == len(strip["tiles"]) - 1
            A = [(image(cur), "r", strip["id"])]
            if pending is not None:
                A.append(("red", "r", pending["id"]))
                folds.append(pending)
            if kind == "dgrad" and last_tile and nxt:
                A.append((image(cur ^ 1), "w", nxt["id"]))
            intervals.append(A)
            barrier()  # B1
            Wi = [("red", "w", tile["id"])]
            pending = tile
            if kind == "fwd" and last_tile and nxt:
                Wi.append((image(cur), "w", nxt["id"]))
            intervals.append(Wi)
            barrier()  # B2
        if kind == "dgrad":
            cur ^= 1
    intervals.append([("red", "r", pending["id"])])
    folds.append(pending)
    return intervals, folds, barriers


def check(kind, run):
    intervals, folds, barriers = replay(kind, run)
    version = {}
    for k, acc in enumerate(intervals):
        read = {b for b, m, _ in acc if m == "r"}
        written = [b for b, m, _ in acc if m == "w"]
        assert not read & set(written), (k, acc)
        assert len(written) == len(set(written)), (k, acc)
        for b, m, tag in acc:
            if m == "r":
                assert version.get(b) == tag, (k, b, version.get(b), tag)
        for b, m, tag in acc:
            if m == "w":
                version[b] = tag
    tiles = [t for s in run for t in s["tiles"]]
    assert [f["id"] for f in folds] == [t["id"] for t in tiles]      # each tile once, in order
    assert [f["outs"] for f in folds] == [t["outs"] for t in tiles]  # with its own base and valid count
    assert len(set(barriers)) == 1
    ntiles = len(tiles)
    assert barriers[0] == (1 + 2 * ntiles if run else 0)
    return intervals, folds


# (Ho, Wo): 30 x 30 two tiles per strip; 9 x 9 one tile per strip and a short last strip; 1 x 1 one pixel
FWD_GEOMS = [(30, 30), (9, 9), (1, 1), (9, 14), (15, 6)]
# first item, number of strips: runs of 1, 2 and 3; starting so that the run crosses a frame
RUNS = [(0, 1), (0, 2), (0, 3), (1, 3)]


@pytest.mark.parametrize("Ho,Wo", FWD_GEOMS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_forward_protocol(Ho, Wo, n):
    spf = (Ho + R - 1) // R
    for first in sorted({0, spf - 1, max(0, spf - 2), 2 * spf - 1}):  # the frame's start, and runs that cross into the next frame
        run = forward_run(first, first + n, Ho, Wo)
        _, folds = check("fwd", run)
        if Ho % 2 and any((it["id"] + 1) % spf == 0 for it in run):  # a short last strip: its valid count differs from a full strip's
            assert any(sum(o["valid"] for t in s["tiles"] for o in t["outs"]) == Wo for s in run)
        if first + n > spf > first:  # a frame change inside the run: bases jump by a frame (more than once where a frame is one strip)
            assert len({f["outs"][0]["base"] // (Ho * Wo * 64) for f in folds}) == (first + n - 1) // spf - first // spf + 1 >= 2
    assert len(forward_run(0, 1, Ho, Wo)[0]["tiles"]) == (2 if 2 * Wo > 32 else 1)


@pytest.mark.parametrize("H,W", [(63, 63), (20, 20), (4, 5), (33, 14)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_data_gradient_protocol_with_two_images(H, W, n):
    spf = ((H + 1) // 2 + R - 1) // R
    for first in sorted({0, spf - 1, max(0, spf - 2), 2 * spf - 1}):
        run = dgrad_run(first, first + n, H, W)
        intervals, folds = check("dgrad", run)
        # the two images alternate: strip i is read from image i & 1, and staged there while strip i - 1 is still being read from the other
        for i, s in enumerate(run):
            reads = {b for acc in intervals for b, m, tag in acc if m == "r" and tag == s["id"] and b.startswith("img")}
            assert reads == {f"img{i & 1}"}
        if H % 2:  # the half-empty last cell row: its odd output row has no extent
            last_rows = [t for s in run for t in s["tiles"] if t["outs"][1]["valid"] == 0]
            assert all(t["outs"][0]["valid"] in (0, W * 32) for t in last_rows)


def test_a_workgroup_without_strips_passes_no_barrier():
    for kind in ("fwd", "dgrad"):
        assert replay(kind, []) == ([], [], [0] * 8)


def test_the_checker_catches_a_stage_inside_the_reading_interval():
    """The forward has one image: staging the next strip in [A] (as the data gradient may, into its other image) must be caught."""
    run = forward_run(0, 2, 30, 30)
    intervals, _, _ = replay("fwd", run)
    bad = [list(a) for a in intervals]
    k = next(i for i, a in enumerate(bad) if ("img", "w", 1) in a)
    bad[k].remove(("img", "w", 1))
    bad[k - 1].append(("img", "w", 1))  # moved from [W] into the [A] in front of it
    assert any({b for b, m, _ in a if m == "r"} & {b for b, m, _ in a if m == "w"} for a in bad)
