"""Batched spike rings restated in numpy — shared by tests/test_delay_batch_cpu.py (which holds the restatement to a brute-force
per-bit loop) and tests/test_delay_batch_gpu.py.  numpy only: nothing here needs a device.

The semantics: ``B`` histories under one head.  ``bits[slot][b]`` holds the packed spikes of sample ``b`` pushed
at a step ``t`` with ``t % depth == slot``; the vector of age ``a`` (0: pushed last) lies in slot ``(head - 1 - a) mod depth``,
history before the first push is silent.  The *unrolled* words of row ``b`` are the bit string of ``ages * n`` bits whose bit
``a * n + i`` is the spike of neuron ``i`` of sample ``b`` at age ``a``, ANDed with bit ``i`` of ``row_mask[a]``; the bits from
``ages * n`` to the end of the row's last word are 0."""
import numpy as np

import delay_cases as DC

__all__ = ['TILES', 'MAX_BATCH', 'batch_ring_np', 'unrolled_words_brute', 'random_mask']

#: the constants of brainevent_amd/csrc/be_delay.hip that the GPU cases are sized by, beside ``delay_cases.TILES``
#: (tests/test_delay_batch_cpu.py ties them to the source text)
TILES = {'kRingMaxBatch': 65535, 'kUnrollThreads': 256}
#: the largest batch: the batch row is the second grid dimension of the push and of the unroll, neither strides over it
MAX_BATCH = TILES['kRingMaxBatch']
#: bits of one output row that one workgroup of the unroll assembles
UNROLL_TILE_BITS = TILES['kUnrollThreads'] * 32


def _active(S):
    S = np.asarray(S)
    return (S > 0) if np.issubdtype(S.dtype, np.floating) else (S != 0)


class batch_ring_np:
    """A list-based history of ``[B, n]`` spike matrices: ``age(a)`` is the matrix pushed ``a`` pushes ago, silent before the
    first push.  ``bits()`` / ``head`` restate the device layout, ``stacked_words`` the unroll."""

    def __init__(self, n, depth, batch):
        self.n, self.depth, self.batch, self.history = int(n), int(depth), int(batch), []

    def push(self, S):
        S = _active(S)
        assert S.shape == (self.batch, self.n)
        self.history.append(S)

    def push_packed(self, words):
        w = np.asarray(words).view(np.uint32).reshape(self.batch, -1)
        self.history.append(np.stack([DC.unpack_words_np(r, self.n)[:self.n] for r in w]))

    head = property(lambda self: len(self.history) % self.depth)

    def age(self, a):
        assert 0 <= a < self.depth
        return self.history[-1 - a] if a < len(self.history) else np.zeros((self.batch, self.n), dtype=bool)

    def bits(self):
        """uint32 ``[depth, B, ceil(n / 32)]``: slot ``t % depth`` holds push ``t`` (the last ``depth`` pushes survive)."""
        out = np.zeros((self.depth, self.batch, (self.n + 31) // 32), dtype=np.uint32)
        for t in range(max(0, len(self.history) - self.depth), len(self.history)):
            out[t % self.depth] = DC.pack_rows_np(self.history[t])
        return out

    def stacked_words(self, ages=None, row_mask=None):
        """uint32 ``[B, ceil(ages * n / 32)]``: the ages side by side, ``n`` bits each, then packed."""
        ages = self.depth if ages is None else ages
        cols = []
        for a in range(ages):
            s = self.age(a)
            if row_mask is not None:
                s = s & DC.unpack_words_np(row_mask[a], self.n)[:self.n]
            cols.append(s)
        return DC.pack_rows_np(np.concatenate(cols, axis=1))


def unrolled_words_brute(bits, head, n, depth, batch, ages, row_mask=None):
    """The contract of ``be_spike_ring_unroll`` bit by bit, from the device layout (``bits [depth, B, W]`` and ``head``)."""
    bits = np.asarray(bits).view(np.uint32).reshape(depth, batch, -1)
    out = np.zeros((batch, (ages * n + 31) // 32), dtype=np.uint32)
    for b in range(batch):
        for p in range(ages * n):
            a, i = divmod(p, n)
            slot = (head - 1 - a) % depth
            bit = (int(bits[slot, b, i // 32]) >> (i % 32)) & 1
            if row_mask is not None:
                bit &= (int(row_mask[a, i // 32]) >> (i % 32)) & 1
            out[b, p // 32] |= np.uint32(bit << (p % 32))
    return out


def random_mask(rng, rows, n):
    """uint32 ``[rows, ceil(n / 32)]`` of random words (bits past ``n`` set at random too: the kernels must not care)."""
    return rng.integers(0, 2 ** 32, (rows, (n + 31) // 32), dtype=np.uint64).astype(np.uint32)
