"""A batch of entities with DIFFERENT numbers of context lines — DESIGN.md §34.

`get_context_indices` (utils/context_utils.py:365-385) pads every entity of a batch to the line count of the batch's richest entity and
`get_mask` (:285-291) marks the first n_u lines of entity u as present.  `RaggedLines` is the same batch without the padding lines: the
context arrays are flat lists of L = sum n_u rows, and entity u owns the rows line_ptr[u] .. line_ptr[u + 1] — what `RaggedAdjacency`
is for graphs of different sizes.

    lines = RaggedLines.from_counts([3, 1, 0, 2], device)        # or .from_mask(context_mask), or ContextBatcher.batch(..., ragged_lines=True)
    out = entity_line_pool_ragged(states, lines, weight, bias)     # states [L, C]

Fields: `line_ptr` int32 [U + 1] on the device, and the host ints `U`, `total` (= L) and `n_max` (the longest entity's lines).  A count of
0 is legal.  `to_mask` and `pad` give the padded form back (for the tests and for the stock-op fallbacks); neither reads the device.
"""
import torch


class RaggedLines:
    __slots__ = ("line_ptr", "U", "total", "n_max", "_rows")

    def __init__(self, line_ptr, U, total, n_max):
        """line_ptr int32 [U + 1] (ascending, line_ptr[0] = 0, line_ptr[U] = total); the three sizes are the caller's word: nothing is read
        back.  `from_counts` and `from_mask` derive them."""
        if not torch.is_tensor(line_ptr) or line_ptr.dtype != torch.int32 or line_ptr.dim() != 1 or line_ptr.numel() != int(U) + 1:
            raise ValueError("RaggedLines: line_ptr must be int32 [U + 1]")
        U, total, n_max = int(U), int(total), int(n_max)
        if U < 0 or not 0 <= n_max <= total <= U * n_max:
            raise ValueError("RaggedLines: need U >= 0 and 0 <= n_max <= total <= U n_max, got U %d, total %d, n_max %d" % (U, total, n_max))
        self.line_ptr, self.U, self.total, self.n_max = line_ptr, U, total, n_max
        self._rows = None

    @classmethod
    def from_counts(cls, counts, device=None):
        """counts: the entities' line counts (a sequence of ints or an integer tensor; a tensor on a GPU is read back once)."""
        if torch.is_tensor(counts):
            if counts.dim() != 1 or counts.is_floating_point() or counts.dtype == torch.bool:
                raise ValueError("RaggedLines.from_counts: counts must be a one-dimensional integer tensor")
            device = counts.device if device is None else device
            counts = counts.tolist()
        counts = [int(c) for c in counts]
        if any(c < 0 for c in counts):
            raise ValueError("RaggedLines.from_counts: a line count below 0")
        ptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
        if int(ptr[-1]) >= 2 ** 31:
            raise ValueError("RaggedLines.from_counts: 2^31 lines or more")
        return cls(ptr.to(dtype=torch.int32, device=device), len(counts), int(ptr[-1]), max(counts) if counts else 0)

    @classmethod
    def from_mask(cls, mask):
        """mask bool [U, P], True = padding line, as get_mask writes it (utils/context_utils.py:285-291): every row must be a prefix of
        present lines followed by padding, else ValueError.  Reads the mask back (the one place where a host read is acceptable)."""
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.dim() != 2:
            raise ValueError("RaggedLines.from_mask: mask must be bool [U, P]")
        counts = (~mask).sum(1)
        prefix = torch.arange(mask.shape[1], device=mask.device)[None, :] >= counts[:, None]
        if not bool(torch.equal(prefix, mask)):
            raise ValueError("RaggedLines.from_mask: a present line behind a padding line (every row must be a prefix of present lines)")
        return cls.from_counts(counts, mask.device)

    def counts(self):
        """int64 [U] on the device: the entities' line counts."""
        ptr = self.line_ptr.to(torch.int64)
        return ptr[1:] - ptr[:-1]

    def to_mask(self, P, k=1):
        """bool [U, P - k + 1], True = padding: position p of entity u (a window of k lines from line p) is present where p + k <= n_u.
        k = 1 is get_mask's mask of the lines."""
        if P - k + 1 < 0:
            raise ValueError("RaggedLines.to_mask: P = %d lines hold no window of k = %d" % (P, k))
        return torch.arange(P - k + 1, device=self.line_ptr.device)[None, :] > (self.counts() - k)[:, None]

    def rows(self):
        """(entity, line) of every row: two int64 [L] on the device, built once."""
        if self._rows is None:
            ptr = self.line_ptr.to(torch.int64)
            r = torch.arange(self.total, device=ptr.device)
            u = torch.searchsorted(ptr[1:].contiguous(), r, right=True)
            self._rows = (u, r - ptr[u])
        return self._rows

    def pad(self, rows, P):
        """[L, ...] -> a zero-filled [U, P, ...] with entity u's rows at [u, :n_u]; differentiable; P >= n_max."""
        if rows.shape[0] != self.total:
            raise ValueError("RaggedLines.pad: %d rows, the batch has %d" % (rows.shape[0], self.total))
        if P < self.n_max:
            raise ValueError("RaggedLines.pad: P = %d is below the longest entity's %d lines" % (P, self.n_max))
        out = rows.new_zeros((self.U, P) + tuple(rows.shape[1:]))
        if self.total == 0:
            return out
        return out.index_put(self.rows(), rows)

    def to(self, device):
        return RaggedLines(self.line_ptr.to(device), self.U, self.total, self.n_max)

    def __repr__(self):
        return "RaggedLines(U=%d, total=%d, n_max=%d, device=%s)" % (self.U, self.total, self.n_max, self.line_ptr.device)
