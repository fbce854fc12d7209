"""Restatement of an open paragraph's host side (include/summertts_hip.h sts_para_open ..; summertts_amd/csrc/para_stream.hpp is the code
under test), in Python integers and written from the definition: the layout continued sentence by sentence, the frontier rule, the
retirement rule and a first-fit pool -- nothing is shared with the header.  The steps themselves are tests/join_stream_ref.py's, of the
FINISHED paragraph."""


class Para:
    def __init__(self, C, Hd, Ho, lead, max_resident, capacity):
        self.C, self.Hd, self.Ho, self.lead = C, Hd, Ho, lead
        self.max_resident, self.capacity = max_resident, capacity
        self.s, self.F = [], []
        self.col = {}                  # resident sentence -> first column
        self.k = 0                     # next undelivered chunk
        self.FJ = None                 # known after finish

    @property
    def E(self):
        return self.s[-1] + self.F[-1] if self.s else 0

    def ready(self):
        """chunks deliverable now: before finish those whose reach (k + 1) C + Ho does not pass E, afterwards all that remain"""
        if self.FJ is not None:
            return max(0, -(-self.FJ // self.C) - self.k)
        n = 0
        while (self.k + n + 1) * self.C + self.Ho <= self.E:
            n += 1
        return n

    def _first_fit(self, used, length):
        run = 0
        for c in range(self.capacity):
            run = 0 if used[c] else run + 1
            if run == length:
                return c + 1 - length
        return -1

    def append(self, F, gap):
        """all or nothing -> list of (start frame, first column) or None"""
        if len(F) > self.max_resident - len(self.col):
            return None
        used = [False] * self.capacity
        for i, c in self.col.items():
            for x in range(c, c + self.F[i]):
                used[x] = True
        placed, e, first = [], self.E, not self.s
        for b, f in enumerate(F):
            start = self.lead if (first and b == 0) else e + gap[b]
            c = self._first_fit(used, f)
            if c < 0:
                return None
            for x in range(c, c + f):
                used[x] = True
            placed.append((start, c))
            e = start + f
        for (start, c), f in zip(placed, F):
            self.col[len(self.s)] = c
            self.s.append(start); self.F.append(f)
        return placed

    def finish(self, trail):
        self.FJ = self.E + trail

    def delivered(self):
        """chunk k has left -> the sentences that retire: those no step from the next chunk on reads"""
        self.k += 1
        done = self.FJ is not None and self.k * self.C >= self.FJ
        out = [i for i in sorted(self.col) if done or self.k * self.C - self.Ho - self.Hd >= self.s[i] + self.F[i]]
        for i in out:
            del self.col[i]
        return out

    def free_frames(self):
        return self.capacity - sum(self.F[i] for i in self.col)
