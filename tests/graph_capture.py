"""Graph capture of stream-ordered entry points (test infrastructure, no fixtures).

_capture(fn): fn captured into one torch.cuda.CUDAGraph after a warm-up on a side stream.

replay_matches_eager(step, mutate, outs, n): the graph of `step`, replayed on changed inputs, against
`step` run eagerly on the same inputs, bit for bit.  What a replay can show that an eager run on the
default stream cannot:
  * a launch on another stream than the current one is not in the graph, so its output does not follow
    the new inputs;
  * a host sync raises during the capture;
  * from the second replay on every temporary of the graph's private pool holds the previous replay's
    bytes, so a temporary read before it is written changes the result.
No tolerance: eager values are pinned to references elsewhere.
"""
import torch

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _capture(fn):
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()   # warm-up on a side stream, as torch.cuda.graphs recommends
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def bits(t):
    """A copy of t as integers of its element size: NaN bit patterns count, -0.0 is not +0.0."""
    return t.detach().contiguous().view(_INT[t.element_size()]).clone()


def snapshot(outs):
    torch.cuda.synchronize()
    return [bits(o) for o in outs]


def first_difference(a, b):
    """None when the two snapshots are the same bits, else a text naming the first output that differs."""
    if len(a) != len(b):
        return f"{len(a)} outputs against {len(b)}"
    for k, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"output {k}: {tuple(x.shape)} {x.dtype} against {tuple(y.shape)} {y.dtype}"
        ne = x != y
        bad = int(ne.sum())
        if bad:
            i = int(torch.nonzero(ne.reshape(-1))[0])
            return (f"output {k}: {bad} of {x.numel()} elements differ, first at flat index {i}: "
                    f"{int(x.reshape(-1)[i]):#x} against {int(y.reshape(-1)[i]):#x}")
    return None


def replay_matches_eager(step, mutate, outs, n=3):
    """step(): the captured function; it refills the list `outs` with its output tensors and runs all
    its work on the current stream.  mutate(i): sets the static inputs, in place, to input set i -- a
    function of i alone.  Rounds 0 .. n - 2 replay on sets 0 .. n - 2, the last round on set 0 again.
      1. set 0, step eagerly: the first eager result;
      2. warm-up and capture;
      3. every round: mutate, replay, then step eagerly on the same inputs -- every output the same bits;
      4. round 1 differs from round 0 in at least one output (else the inputs never reached the graph);
      5. the last round (set 0 after the other sets) is the first eager result, bit for bit."""
    assert n >= 3
    mutate(0)
    step()
    first = snapshot(outs)
    graph = _capture(step)
    static = list(outs)   # the capture's own outputs: a replay rewrites these, an eager step rebinds `outs`
    assert len(static) == len(first) and len(static) > 0
    replays = []
    for i in range(n):
        s = i if i < n - 1 else 0
        mutate(s)
        graph.replay()
        replayed = snapshot(static)
        step()
        eager = snapshot(outs)
        d = first_difference(replayed, eager)
        assert d is None, f"round {i} (input set {s}): replay against eager: {d}"
        replays.append(replayed)
    assert first_difference(replays[0], replays[1]) is not None, \
        "rounds 0 and 1 gave the same bits in every output: the new inputs never reached the graph"
    d = first_difference(replays[-1], first)
    assert d is None, f"set 0 replayed after the other sets against the first eager result: {d}"
    return graph
