"""``DataRepresentation``: the contract every weight-matrix container shares (reference ``brainevent/_data.py:35-230``,
minus ``brainunit.sparse.SparseMatrix`` and the pytree plumbing).

A container carries named *buffers* — per-matrix, non-differentiable state that travels with it, e.g. the scatter plan a
``CSR`` builds on first use (the reference keeps its task workspace there, ``_csr/main.py:148-161``) — and declares the
structure operations of a generic sparse weight matrix; a family that cannot support one refuses it explicitly."""
from typing import Dict, Optional

__all__ = ['DataRepresentation']


class DataRepresentation:
    """Base of ``CSR`` / ``CSC``, ``FixedNumPerPre`` / ``FixedNumPerPost``, the ``JITC*`` matrices and ``Dense``.

    ``buffers`` is a plain dict here (the reference exposes the registered names through a property of the same name);
    ``register_buffer`` / ``set_buffer`` keep the reference's semantics: a buffer has to be registered before it is set."""

    buffers: Dict
    # a numpy array on the LEFT of ``@`` defers to the container's ``__rmatmul__`` instead of treating it as a 0-d object
    __array_ufunc__ = None

    def _init_buffers(self, buffers: Optional[Dict]) -> None:
        if buffers is not None and not isinstance(buffers, dict):
            raise AssertionError("buffers must be a dictionary of name-value pairs.")
        self.buffers = dict(buffers) if buffers else {}

    def register_buffer(self, name, value=None):
        """Register a named buffer with a default value."""
        self.buffers[name] = value

    def set_buffer(self, name, value):
        """Update the value of a previously registered buffer."""
        if name not in self.buffers:
            raise ValueError(f"Buffer '{name}' not registered. Call register_buffer first.")
        self.buffers[name] = value

    # ---- common-API contract: declared here, overridden (or deliberately refused) by the families
    @classmethod
    def fromdense(cls, *args, **kwargs):
        raise NotImplementedError(f"{cls.__name__}.fromdense")

    def todense(self):
        raise NotImplementedError(f"{type(self).__name__}.todense")

    def tocoo(self):
        raise NotImplementedError(f"{type(self).__name__}.tocoo")

    def tocsr(self):
        raise NotImplementedError(f"{type(self).__name__}.tocsr")

    def tocsc(self):
        raise NotImplementedError(f"{type(self).__name__}.tocsc")

    def with_data(self, data):
        raise NotImplementedError(f"{type(self).__name__}.with_data")

    def transpose(self, axes=None):
        raise NotImplementedError(f"{type(self).__name__}.transpose")

    def dt2t(self, y_dim_arr, w_dim_arr):
        """Per-synapse ``w * y`` with ``y`` indexed by the row (pre axis) of the matrix (reference ``_data.py``, the ``dt2t``
        protocol; ``brainevent_amd._dt2t``)."""
        raise NotImplementedError(f"{type(self).__name__}.dt2t")

    def dt2t_transposed(self, y_dim_arr, w_dim_arr):
        """Per-synapse ``w * y`` with ``y`` indexed by the column (post axis) of the matrix."""
        raise NotImplementedError(f"{type(self).__name__}.dt2t_transposed")

    def solve(self, b, tol=1e-6, reorder=1, **kwargs):
        """Solve ``A x = b`` (``brainevent_amd._solve``); served by CSR, CSC and ``Dense``."""
        raise NotImplementedError(f"{type(self).__name__}.solve: linear systems are served by CSR, CSC and Dense only.")

    def __getitem__(self, index):
        """Rows of the matrix as a dense array (``brainevent_amd._slice``); served by the four stored-rows containers and
        ``Dense``."""
        raise NotImplementedError(f"{type(self).__name__}.__getitem__: row slicing is served by CSR, CSC, FixedNumPerPre, "
                                  f"FixedNumPerPost and Dense only.")

    def slice_rows(self, index):
        """``W[rows, :]`` as a sparse matrix (``brainevent_amd._slice``)."""
        raise NotImplementedError(f"{type(self).__name__}.slice_rows: row slicing is served by CSR, CSC, FixedNumPerPre and "
                                  f"FixedNumPerPost only.")
