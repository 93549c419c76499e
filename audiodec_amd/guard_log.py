"""The log of the DEFERRED guard, free of torch / HIP: what is unverified, when the host waits, what a repair is handed.

The product arithmetic is split-f16; a program step that met an operand beyond the f16 range says so in its program's sticky word.
Behind every step a post is recorded (``adk_program_flags_post``: nothing waits) and the step is logged as ``(program, frames, ticket)`` in
an ENTRY -- any object with ``.steps``: a batch of ``pipeline.StreamingPipeline``, a direct call of ``lazy_guard.CallLog``.  ``GuardLog``
keeps the unverified entries, oldest first, and is the only place that polls:

  * ``collect()`` reads the posts of the head entry that have completed and retires entries whose posts all read 0 (an entry without
    steps -- quantize, lookup -- is retired when it reaches the head); it WAITS for the head only when asked to (``block``) or when the
    log is full for the entry about to be issued: ``depth`` entries pending, a program's unread hops beyond what its rings can be rewound
    by (``budget``), or a program's unread posts beyond the ``POST_SLOTS`` events the native side keeps.
  * A poll reads AND clears the program's word (ABI 14), so a wait and the read of its word are one call, and a word that was read is
    handed on, never dropped.  A word may already hold what a LATER step of the program reported: the blame can only be early.
  * On a non-zero word (``_recover``): drain, read and clear every remaining word, clear the log and hand the entries -- all from the
    head on: it is the first bad one --, the words by program and the culprit (the first reporter of the head entry, in issue order:
    programs behind it, and all of them in later entries, may only have seen its garbage) to the user's ``repair``.

``rewind_and_demote`` is the half of a repair the two users share; how the entries are run again is theirs.
"""
import collections

from . import native

POST_SLOTS = native.POST_SLOTS       # events of posts the native side keeps per program: a ticket older than that cannot be polled any more


def _poll_program(prog, ticket, block):
    return prog.poll_flags(ticket, block)


class GuardLog:
    """`poll(program, ticket, block) -> (done, flags)` (default: the program's own); `repair(entries, flags_by_program, culprit)` is called
    with the unverified entries (oldest first, the first one bad), everything drained, and must leave them correct."""

    def __init__(self, depth, poll, repair, drain, budget=None):
        """depth: most entries unverified at a time; budget: most hops a program may have unread -- what its rings can be rewound by --;
        None = no limit (but a collect() may bring the limit of the programs it is asked about)."""
        assert depth >= 1
        self.depth, self._poll, self._repair, self._drain = int(depth), poll or _poll_program, repair, drain
        self.budget = budget
        self.pending = collections.deque()
        self._hops = {}              # program -> hops of its steps in `pending` (what a repair would have to rewind)
        self._posts = {}             # program -> posts of its steps in `pending` (events the native side has to keep)
        self.verified = 0            # entries found clean (or repaired) so far
        self.repairs = 0
        self.waits = 0               # times the host had to wait for a post of the oldest entry (log full)

    # (push / _full / collect run once per direct call on the host's issue path -- four times per frame for a single stream, where the host,
    # not the device, sets the pace: plain loops and running counts per program, nothing that walks the whole log)
    def push(self, entry):
        hops, posts = self._hops, self._posts
        for prog, frames, _t in entry.steps:
            hops[prog] = hops.get(prog, 0) + frames
            posts[prog] = posts.get(prog, 0) + 1
        self.pending.append(entry)

    def units_pending(self):
        """Most hops any one program would have to be rewound by."""
        return max(self._hops.values(), default=0)

    def _full(self, incoming, progs, posts, budget):
        if len(self.pending) >= self.depth:
            return True
        hops, nposts = self._hops, self._posts
        for p in (hops if progs is None else progs):
            if nposts.get(p, 0) + posts > POST_SLOTS or (budget is not None and hops.get(p, 0) + incoming > budget):
                return True
        return False

    def collect(self, block=False, incoming=0, progs=None, posts=1, budget=None):
        """Retire the entries whose posts have completed; block=True -- or a log that is full for an entry about to be issued that steps each
        of `progs` (None: every program in the log) by `incoming` hops in `posts` steps -- waits for the oldest first.  budget: the hop limit
        of `progs`, where it is theirs and not the log's."""
        pending, poll, hops, nposts = self.pending, self._poll, self._hops, self._posts
        if budget is None:
            budget = self.budget
        while pending:
            e = pending[0]
            found, ready = None, True
            for prog, _frames, ticket in e.steps:
                done, fl = poll(prog, ticket, block)
                if not done:
                    if not self._full(incoming, progs, posts, budget):
                        ready = False
                        break
                    self.waits += 1
                    done, fl = poll(prog, ticket, True)
                if fl:
                    if found is None:
                        found = []
                    found.append((prog, fl))
            if found is not None:
                self._recover(found)                     # (what was read is gone from the words: handed on; _recover reads the rest)
                return
            if not ready:
                return
            pending.popleft()
            for prog, frames, _t in e.steps:
                hops[prog] -= frames
                nposts[prog] -= 1
            self.verified += 1

    def _recover(self, found):
        """found: [(program, flags)] read from posts of the OLDEST unverified entry, in issue order: that entry is the first bad one."""
        self._drain()                                   # everything issued has finished: every post can be read
        entries = list(self.pending)
        by_prog, culprit = {}, found[0][0]
        for prog, fl in found:
            by_prog[prog] = by_prog.get(prog, 0) | fl
        for e in entries:                               # the rest of the words: read (and thereby cleared) too
            for prog, _frames, ticket in e.steps:
                _done, fl = self._poll(prog, ticket, True)
                if fl:
                    by_prog[prog] = by_prog.get(prog, 0) | fl
        self.pending.clear()
        self._hops.clear()
        self._posts.clear()
        self._repair(entries, by_prog, culprit)
        self.verified += len(entries)
        self.repairs += 1


def rewind_and_demote(entries, by_prog, culprit, who):
    """The first half of a repair (GuardLog's `repair` arguments): any flag but the f16 overflow raises; every program is taken back by the
    steps it took for `entries`, newest first; the culprit is replaced by its exact-f32 twin.  The caller then runs the entries again."""
    other = 0
    for fl in by_prog.values():
        other |= fl & ~native.FLAG_F16_OVERFLOW
    native.raise_for_flags(other, who)
    for e in reversed(entries):
        for prog, frames, _t in reversed(e.steps):
            prog.rewind(frames)
    if not by_prog.get(culprit, 0) & native.FLAG_F16_OVERFLOW or not culprit.split16 or culprit.twin_builder is None or culprit.demoted:
        raise native.NativeError(f"{who}: a program without an exact-f32 twin reported an f16 range overflow")
    culprit.demote()
