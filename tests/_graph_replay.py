"""The hipGraph replay protocol, once ("Replaying the library from a captured hipGraph").

include/apa.h promises that every launch goes to the stream it is given, without synchronisation or allocation, so that
every entry point can be captured.  `replay_equals_eager` holds one entry point (or a short sequence of them) to that:
R eager calls on one instance, then ONE captured call on a second, identical instance (warmed up once on a side stream
and put back to its initial state first) replayed R times, with the mutable inputs rewritten IN PLACE before every
call -- and every output and every piece of written state of replay r equal to
that of eager call r by torch.equal ("identical calls give identical bits"; a replay is the same launches with the same
arguments).  A `Case` may name a float64 bound for an output that accumulates with floating-point atomics instead.
"""
import pytest
import torch

SENTINEL = 0x5B          # every byte of an output before the capture: finite in f32 / bf16 / fp8, no valid id or label


class Case(object):
    """What `make()` returns.
    call     enqueues the entry point(s) on torch's CURRENT stream; may return {name: tensor} for results a functional
             wrapper allocates (under capture they live in the graph's pool: the tensors of the capture are read after
             every replay)
    inputs   {name: tensor}: what the rounds rewrite in place
    state    {name: tensor}: every caller-owned output and every piece of state the call writes (weights, accumulators,
             the dropout counter, cache.status, tags, workspaces the caller must keep)
    outputs  names of `state` the call overwrites completely: pre-filled with SENTINEL bytes before the capture
    main     the name, or names, (in `state` or in call()'s result) whose rounds 0 and 1 must differ: outputs that can
             differ only through the rewritten inputs where the row has such (cache.status, scores without dropout)
    after    f(r, snapshot) called after eager call r: what the row knows about its state (the counter advanced, ...)
    bounds   {name: f(got, r)}: outputs held to a float64 bound by f (which asserts) and not to bits"""

    def __init__(self, call, inputs, state, outputs=(), main=None, bounds=None, after=None):
        self.call, self.inputs, self.state = call, dict(inputs), dict(state)
        self.outputs, self.bounds, self.after = tuple(outputs), dict(bounds or {}), after
        self.main = (main,) if isinstance(main, str) else tuple(main or ())
        for k in self.outputs:
            assert k in self.state, k


def _sync(what):
    """a device fault ends the session: nothing else is started on a card that has faulted"""
    try:
        torch.cuda.synchronize()
    except Exception as e:     # noqa: BLE001 -- whatever the runtime raises for a fault
        pytest.exit('%s: the device reported %r; no further test is started' % (what, e), returncode=3)


def _write(case, values):
    for k, v in values.items():
        case.inputs[k].copy_(v)


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def _fill_sentinel(t):
    t.view(-1).view(torch.uint8).fill_(SENTINEL)


def _compare(name, case, got, want, r):
    for k, w in want.items():
        g = got[k]
        if k in case.bounds:
            case.bounds[k](g, r)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, '%s: %s changed its shape' % (name, k)
        assert torch.equal(g, w), '%s: replay %d differs from eager call %d in %r' % (name, r, r, k)


def _prepared(name, make, first_round):
    """A fresh instance, warmed up once on a side stream (lazy function attributes, first-call allocations), then put
    back to its initial state in place: the instance a call is captured on."""
    c = make()
    init_inputs, init_state = _clone(c.inputs), _clone(c.state)
    _write(c, first_round)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.call()
    torch.cuda.current_stream().wait_stream(side)
    _sync(name)
    for k, v in init_inputs.items():
        c.inputs[k].copy_(v)
    for k, v in init_state.items():
        c.state[k].copy_(v)
    _sync(name)
    return c


def replay_equals_eager(name, make, rounds, R=3, frozen=False):
    """`rounds[r]`: {input name: tensor} written in place (copy_) before call r.  `frozen`: the entry point reads no
    input from HBM (every argument travels by value), so all rounds are the same call and step 6 does not apply.
    Returns the eager results."""
    assert len(rounds) >= R >= 2
    # 1. the eager pass
    a = make()
    eager = []
    for r in range(R):
        _write(a, rounds[r])
        ret = a.call() or {}
        _sync(name)
        snap = _clone(a.state)
        assert not set(ret) & set(snap), '%s: a result shadows a piece of state' % name
        snap.update(_clone(ret))
        eager.append(snap)
        if a.after is not None:
            a.after(r, snap)
    # 6. a replay that ignored its rewritten inputs must not pass
    assert a.main and all(m in eager[0] for m in a.main), (name, a.main)
    for m in a.main:
        assert frozen != (not torch.equal(eager[0][m], eager[1][m])), \
            '%s: rounds 0 and 1 give %s %r' % (name, 'different' if frozen else 'the same', m)
    del a
    # 2. a fresh instance with identical initial state, warmed up and restored; outputs pre-filled with the sentinel
    b = _prepared(name, make, rounds[0])
    for k in b.outputs:
        _fill_sentinel(b.state[k])
    _write(b, rounds[0])
    _sync(name)
    before = _clone(b.state)
    # 3. one captured call: single stream, linear
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            ret = b.call() or {}
    except Exception as e:     # torch.cuda.graph has ended the capture
        _sync(name)
        raise AssertionError('%s: the capture failed: %s: %s' % (name, type(e).__name__, e)) from e
    _sync(name)
    # 4. capturing must not execute
    for k, v in before.items():
        assert torch.equal(b.state[k], v), '%s: %r was written while capturing' % (name, k)
    # 5. the replays
    for r in range(R):
        _write(b, rounds[r])
        graph.replay()
        _sync(name)
        got = dict(b.state)
        got.update(ret)
        assert set(got) == set(eager[r]), (name, sorted(got), sorted(eager[r]))
        _compare(name, b, got, eager[r], r)
    return eager
