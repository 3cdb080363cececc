"""Stand-in for the `dgl` package, for the golden-vector generators only: the reference's transformer
path imports dgl.sparse and calls four things from it (tests/golden/_stubs/dgl/sparse.py)."""
from . import sparse  # noqa: F401
