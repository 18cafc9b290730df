"""The session recorder's page machine (csrc/tip_record.hip; include/tip_hip.h, "session recorder") restated in numpy: open / append /
close / drain over a schedule, with the same pool size, the same drop rule and the same gap records — and, beside it, the plain truth
of every session (the rows that were stored, in order; where rows were dropped, and how many), kept without any page at all.

The device does not define WHICH slots get a page when fewer are free than slots ask for one in the same frame.  The oracle refuses
such a frame (Contention): a schedule that is to be compared bit for bit must not contain one."""
import collections

import numpy as np

S_OPEN, S_SESSION, S_ROWS, S_PAGE, S_FILL, S_DROPPED, S_GAPS, S_GAP = range(8)
R_SLOT, R_SESSION, R_SEQ, R_ROWS, R_GAP = range(5)


class Contention(AssertionError):
    pass


class Truth:
    def __init__(self, slot, width):
        self.slot, self.rows, self.gaps, self.dropped, self.pending, self.width = slot, [], [], 0, 0, width

    def stored(self, row):
        if self.pending:
            self.gaps.append((len(self.rows), self.pending))
            self.pending = 0
        self.rows.append(np.array(row, dtype=np.float32))

    def lost(self):
        self.pending += 1
        self.dropped += 1

    def final(self):
        """(rows [L, W], gaps, dropped) — a run of drops behind the last stored row is a gap at row L."""
        rows = np.stack(self.rows) if self.rows else np.zeros((0, self.width), np.float32)
        return rows, self.gaps + ([(len(self.rows), self.pending)] if self.pending else []), self.dropped


class RecordOracle:
    def __init__(self, n, pages, page_rows, width):
        self.n, self.P, self.R, self.W = n, pages, page_rows, width
        self.heads = np.zeros((n, 8), np.int32)
        self.heads[:, S_PAGE] = -1
        self.recs = np.zeros((pages, 8), np.int32)
        self.recs[:, R_SLOT] = -1
        self.free = collections.deque(range(pages))
        self.full = collections.deque()
        self.data = np.zeros((pages, page_rows, width), np.float32)
        self.truth = {}                                         # session id -> Truth

    def open(self, slots, sessions):
        for slot, sid in zip(slots, sessions):
            if 0 <= slot < self.n and not self.heads[slot, S_OPEN]:
                self.heads[slot] = (1, sid, 0, -1, 0, 0, 0, 0)
                self.truth[sid] = Truth(slot, self.W)

    def close(self, slots):
        for slot in slots:
            if 0 <= slot < self.n and self.heads[slot, S_OPEN]:
                h = self.heads[slot]
                if h[S_PAGE] >= 0:
                    self.full.append(int(h[S_PAGE]))
                h[S_PAGE], h[S_FILL], h[S_OPEN] = -1, 0, 0

    def append(self, rows, valid=None, valid_min=1):
        """rows [n, W]: what the sources hold this frame."""
        live = [s for s in range(self.n) if self.heads[s, S_OPEN] and (valid is None or valid[s] >= valid_min)]
        asking = [s for s in live if self.heads[s, S_PAGE] < 0]
        if 0 < len(self.free) < len(asking):
            raise Contention(f"{len(asking)} slots ask for a page and {len(self.free)} are free: the device's outcome is not defined")
        for s in live:
            h = self.heads[s]
            t = self.truth[int(h[S_SESSION])]
            if h[S_PAGE] < 0:
                if not self.free:
                    if h[S_GAP] == 0:
                        h[S_GAPS] += 1
                    h[S_GAP] += 1
                    h[S_DROPPED] += 1
                    t.lost()
                    continue
                page = self.free.popleft()
                self.recs[page, :5] = (s, h[S_SESSION], h[S_ROWS] // self.R, 0, h[S_GAP])
                h[S_GAP], h[S_PAGE], h[S_FILL] = 0, page, 0
            page = int(h[S_PAGE])
            self.data[page, h[S_FILL]] = rows[s]
            t.stored(rows[s])
            h[S_FILL] += 1
            h[S_ROWS] += 1
            self.recs[page, R_ROWS] = h[S_FILL]
            if h[S_FILL] == self.R:
                self.full.append(page)
                h[S_PAGE], h[S_FILL] = -1, 0

    def drain(self, max_pages):
        """-> (records [k, 8], contents [k, R, W], pages still queued, pages in use afterwards)."""
        k = min(len(self.full), max_pages)
        pages = [self.full.popleft() for _ in range(k)]
        recs, body = self.recs[pages].copy().reshape(k, 8), self.data[pages].copy().reshape(k, self.R, self.W)
        self.free.extend(pages)
        return recs, body, len(self.full), self.P - len(self.free)

    def totals(self):
        return {"rows_written": int(self.heads[:, S_ROWS].sum()), "rows_dropped": int(self.heads[:, S_DROPPED].sum()),
                "gaps": int(self.heads[:, S_GAPS].sum()), "pages_in_use": self.P - len(self.free), "pages": self.P}
