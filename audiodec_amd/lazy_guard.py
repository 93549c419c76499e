"""The guard of DIRECT calls: checked when a result is first looked at, not when it is computed.

The reference's callers drive the model objects one call at a time -- ``encode``, ``quantize``, ``lookup``, ``decode``
(demoFile.py:58-61, utils/audiodec.py:100-106, bin/stream.py:212-239).  Until round 5 the guard of such calls
was synchronous: one 1-thread kernel + one stream synchronisation per program step before the next call could even be
enqueued (``_StreamBase._step``), i.e. the host's enqueue time of every call was exposed and three HIP streams could not
overlap -- 183 k frames/s against 271 k for ``pipeline.StreamingPipeline``, whose guard is deferred.

Here the same deferral for direct calls.  A generator's public call

  * posts the flag word of every program step behind the step (``adk_program_flags_post``: nothing waits),
  * records itself in a ``CallLog`` -- what it stepped, the tensors it read and wrote, how to run it again --,
  * returns its result as a ``GuardedTensor``: an ordinary ``torch.Tensor`` (same storage) whose every use through torch --
    ``.cpu()``, ``.to()``, ``.numpy()``, ``data_ptr()``, indexing, arithmetic, printing, ``record_stream`` ... -- first SETTLES
    the log: waits for the posts of everything recorded so far and, if one reports an f16 range overflow, repairs (below).
    A result can therefore not leave the device, or be looked at by anything but this library, unverified; ``.cpu()`` waits
    for the stream anyway, so the check costs a caller that reads its results nothing, and a caller that only hands them on
    to the next call of this library (``quantize(encode(x))``) nothing either: a guarded tensor of the SAME log is taken as
    it is, its verification is implied by the order of the log.  A guarded tensor of ANOTHER log (the codes of a
    transmitter arriving at a receiver on another device) settles its log first.

The log itself -- which calls are unverified, the one loop that polls, when a call waits for the oldest one (a program's rings
could not be rewound by one more call, its unread posts would outnumber the events the native side keeps, or ``MAX_PENDING``
calls are pending), what a failure hands to the repair -- is ``guard_log.GuardLog``, the same one ``pipeline.StreamingPipeline``
keeps its batches in.  ``CallLog`` is that log with calls as entries: it adds the lock, ``run()`` and the redo.

Repair: ``GuardLog._recover`` drains the device and reads every word; ``guard_log.rewind_and_demote`` rewinds every program
step of every unverified call (newest first) and demotes the program that reported first to its exact-f32 twin -- both as for
the batches of a pipeline; ``CallLog._redo`` then runs the calls again in order, each with the generators' synchronous guard,
into the tensors the callers already hold (later calls read the earlier calls' outputs through those very tensors).  A call
whose inputs all came from outside repeats with ``ADK_STEP_REPLAY`` (its input rows are still in the program's first ring: the
caller may have reused its input tensor); a call that read results of this log re-writes its input ring from the repeated
results.  One ``RuntimeWarning``, no exception.

One log is shared by the generators of an ``AudioDec`` object on one device.  A lock makes it safe for the reference
streamer's transmitter / receiver threads: while one thread repairs, ``in_redo`` names it -- its own repeated calls and looks
bypass the log --, and any other thread's look or call waits on the lock until the repair is over and is then handled as
usual.  ``pipeline.StreamingPipeline`` bypasses the call log (it owns the guard of its batches).
``ADK_GUARD_MODE=sync`` / ``set_guard(True, mode="sync")`` keeps the synchronous check of rounds 3-5.
"""
import threading
import warnings

import torch

from .guard_log import POST_SLOTS, GuardLog, rewind_and_demote

MAX_PENDING = 64          # calls a log keeps unverified at most (entries without program steps -- quantize, lookup -- count too)


def plain(t):
    """The ordinary tensor behind a GuardedTensor (same storage), WITHOUT settling its log; anything else as it is."""
    if type(t) is GuardedTensor:
        p = t.__dict__.get("_adk_plain")
        if p is not None:
            return p
        with torch._C.DisableTorchFunctionSubclass():
            return t.as_subclass(torch.Tensor)
    return t


def log_of(t):
    return t.__dict__.get("_adk_log") if type(t) is GuardedTensor else None


def settled(t):
    """The ordinary tensor behind `t` once its log, if it has one, has verified everything recorded so far."""
    lg = log_of(t)
    if lg is not None:
        lg.settle()
    return plain(t)


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _tensors(o)


class GuardedTensor(torch.Tensor):
    """A result of a guarded direct call.  Shares the storage of the tensor the kernels wrote; any torch function applied to it
    settles the CallLog it belongs to first and then runs on the plain tensor (results are plain tensors)."""

    @staticmethod
    def wrap(t, log):
        g = torch.Tensor._make_subclass(GuardedTensor, t)
        g.__dict__["_adk_log"] = log
        g.__dict__["_adk_plain"] = t            # (what the kernels wrote into: handing a result on to the next call costs a dict lookup)
        return g

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        seen = set()
        for a in list(_tensors(args)) + list(_tensors(kwargs)):
            lg = log_of(a)
            if lg is not None and id(lg) not in seen:
                seen.add(id(lg))
                lg.settle()
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


class _Call:
    __slots__ = ("gen", "impl", "args", "out", "steps", "replay")

    def __init__(self, gen, impl, args, out, steps, replay):
        self.gen, self.impl, self.args, self.out, self.steps, self.replay = gen, impl, args, out, steps, replay


class CallLog(GuardLog):
    """Unverified direct calls of the generators that share this log, oldest first (see the module docstring): a GuardLog whose entries
    are calls, behind a lock."""

    def __init__(self, device=None, drain=None):
        """device: the HIP device of the generators that share the log; drain() (tests) replaces the device synchronisation of a repair."""
        self.device = device
        super().__init__(MAX_PENDING, None, self._redo,
                         drain if drain is not None else (lambda: torch.cuda.synchronize(device) if device is not None else torch.cuda.synchronize()))
        self.lock = threading.RLock()
        self.in_redo = None        # the thread that is repeating calls in a repair (its own calls and looks bypass the log), else None

    def settle(self):
        """Every call recorded so far is verified (and repaired if need be) when this returns.  A thread other than the repairing one waits
        for the repair on the lock."""
        if self.in_redo is not None and self.in_redo == threading.get_ident():
            return
        with self.lock:
            if self.pending:
                self.collect(block=True)

    # ---- one guarded call ----
    def run(self, gen, impl, args, progs, frames, external_replay=True):
        """impl(*plain args) with the guard deferred; returns the result as a GuardedTensor of this log.  progs: the programs the call
        steps, frames: by how many hops (0: none -- quantize / lookup)."""
        with self.lock:
            own = False
            pargs = []
            for a in args:
                if type(a) is GuardedTensor:
                    d = a.__dict__
                    lg = d.get("_adk_log")
                    if lg is self:
                        own = True
                    elif lg is not None:
                        lg.settle()
                    pa = d.get("_adk_plain")
                    a = pa if pa is not None else plain(a)
                pargs.append(a)
            posts, budget = 1, None
            for p in progs:                                  # (every caller steps ONE program per call)
                budget = (p.rewind_depth + 1) * p.max_frames     # hops the program's rings can be rewound by
                if frames > p.max_frames:
                    posts = -(-frames // p.max_frames)       # program steps, i.e. posts, of this call
                    if frames > budget or posts > POST_SLOTS:
                        # longer than the rings can be rewound by, or than the native side keeps events for (a whole utterance in one
                        # call): checked synchronously, step by step
                        self.settle()
                        return impl(*pargs)
            if self.pending:
                self.collect(False, frames, progs, posts, budget)
            steps = []
            gen._defer = steps
            try:
                out = impl(*pargs)
            finally:
                gen._defer = None
            self.push(_Call(gen, impl, pargs, out, steps, external_replay and not own))
            return GuardedTensor.wrap(out, self)

    # ---- repair ----
    def _redo(self, calls, by_prog, culprit):
        """GuardLog's repair: everything is drained and the log is empty; `calls` are run again, in order, into the tensors handed out."""
        rewind_and_demote(calls, by_prog, culprit, "guarded call")
        self.in_redo = threading.get_ident()
        try:
            with torch.no_grad():
                for c in calls:
                    c.gen._replay = bool(c.replay)
                    try:
                        new = c.impl(*c.args)          # gen._defer is None and this thread is in redo: the generators' synchronous guard checks every step
                    finally:
                        c.gen._replay = False
                    if new.data_ptr() != c.out.data_ptr():
                        c.out.copy_(new.reshape(c.out.shape))
            self._drain()
        finally:
            self.in_redo = None
        warnings.warn(f"an operand left the f16 range (|v| > 65504) in a split-f16 conv; the last {len(calls)} call(s) were repeated with the exact-f32 "
                      "kernels for the program concerned, which continues on them", RuntimeWarning, stacklevel=5)
