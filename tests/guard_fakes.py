"""The fake program of the CPU guard tests (test_pipeline_guard.py, test_lazy_guard.py), with the native side's semantics
(adk_program_flags_post / adk_program_flags_poll, ABI 14): ONE sticky word per program; a poll that completes returns, AND CLEARS,
everything the posts up to the fake device clock reported; only the events of the last POST_SLOTS posts are kept."""
from audiodec_amd import native


class FakeProgram:
    """Posts complete when the fake device clock (`completed`: tickets <= it are done) has passed them; a blocking poll moves the clock to
    its ticket, no further.  `fail_at[ticket]` is what the step before that post reports into the word."""

    def __init__(self, name, rewind_depth=4, max_frames=1, events=None):
        self.name, self.rewind_depth, self.max_frames = name, rewind_depth, max_frames
        self.tickets, self.completed, self.fail_at = 0, -1, {}
        self.blocked = 0
        self._read = -1              # the word holds what the posts in (_read, completed] reported
        self._polled = -1            # newest ticket a completed poll was made for
        self.most_unread = 0         # most posts ever outstanding behind the newest polled one
        self.split16, self.twin_builder, self.demoted = True, object(), False
        self.events = events if events is not None else []

    def post(self):
        t = self.tickets
        self.tickets += 1
        self.most_unread = max(self.most_unread, self.tickets - 1 - self._polled)
        return t

    def poll_flags(self, ticket, block):
        if ticket < 0 or ticket >= self.tickets or ticket + native.POST_SLOTS < self.tickets:
            raise native.NativeError("program_flags_poll: unknown ticket, or more than ADK_POST_SLOTS posts since it was issued")
        if ticket > self.completed:
            if not block:
                return False, 0
            self.blocked += 1
            self.completed = ticket      # waiting lets the device get there
        word = 0
        for t in range(self._read + 1, self.completed + 1):
            word |= self.fail_at.get(t, 0)
        self._read = max(self._read, self.completed)
        self._polled = max(self._polled, ticket)
        return True, word

    poll = poll_flags

    def rewind(self, frames):
        self.events.append(("rewind", self.name, frames))

    def demote(self):
        self.events.append(("demote", self.name))
        self.split16, self.demoted = False, True
