"""Stand-in for dgl.sparse written from DGL's documented semantics, in plain torch (differentiable,
any dtype): the four things the reference's transformer path calls.

  spmatrix(indices, val=None, shape=None)  COO matrix; indices [2, nnz] = (row, col); val defaults to
                                           ones; duplicate entries stay separate entries
  bsddmm(A, X1, X2)                        A (L, M), X1 (L, N, K), X2 (N, M, K) -> sparse (L, M) with
                                           vector values: val[e, k] = A.val[e] · Σ_n X1[row_e, n, k] X2[n, col_e, k]
  SparseMatrix.softmax(dim=1)              softmax over the non-zero entries of each row, per value component
  bspmm(A, X)                              A (L, M) with values (nnz, K), X (M, N, K) -> (L, N, K):
                                           out[i, n, k] = Σ_{e: row_e = i} A.val[e, k] X[col_e, n, k]
"""
import torch


class SparseMatrix:
    def __init__(self, row, col, val, shape):
        self.row, self.col, self.val, self.shape = row, col, val, tuple(shape)

    @property
    def nnz(self):
        return self.row.numel()

    def softmax(self, dim=1):
        assert dim == 1, "softmax over the entries of each row"
        val = self.val
        idx = self.row.view(-1, *([1] * (val.dim() - 1))).expand_as(val)
        top = torch.full((self.shape[0],) + tuple(val.shape[1:]), float("-inf"), dtype=val.dtype, device=val.device)
        top = top.scatter_reduce(0, idx, val.detach(), "amax")
        w = torch.exp(val - top[self.row])
        den = torch.zeros_like(top).index_add(0, self.row, w)
        return SparseMatrix(self.row, self.col, w / den[self.row], self.shape)


def spmatrix(indices, val=None, shape=None):
    row, col = indices[0].long(), indices[1].long()
    if shape is None:
        shape = (int(row.max()) + 1, int(col.max()) + 1)
    if val is None:
        val = torch.ones(row.numel(), device=row.device)
    return SparseMatrix(row, col, val, shape)


def bsddmm(A, X1, X2):
    assert X1.dim() == 3 and X2.dim() == 3 and X1.shape[0] == A.shape[0] and X2.shape[1] == A.shape[1]
    # val[e, k] = Σ_n X1[row_e, n, k] X2[n, col_e, k]
    prod = (X1[A.row] * X2.permute(1, 0, 2)[A.col]).sum(1)
    scale = A.val.to(prod.dtype)
    return SparseMatrix(A.row, A.col, prod * (scale[:, None] if scale.dim() == 1 else scale), A.shape)


def bspmm(A, X):
    assert X.dim() == 3 and X.shape[0] == A.shape[1] and A.val.dim() == 2
    msg = A.val[:, None, :] * X[A.col]
    return torch.zeros((A.shape[0],) + tuple(X.shape[1:]), dtype=msg.dtype, device=msg.device).index_add(0, A.row, msg)
