"""The float64 oracle of the KPConv stem (tests/test_kpconv_cpu.py, tests/test_kpconv_hip.py): torch on the CPU, written from the three
formulas of torch_points3d 1.3.0's rigid KPConv with linear influence and sum aggregation (third party: parity unpinned):

    w[i,k,n]  = max(0, 1 - || (support[j] - query[i]) - K_points[k] ||_2 / e)   if 0 <= j = neighbors[i,n] < n_s, else 0
    wf[i,k,:] = sum_n w[i,k,n] * x[j,:]
    out[i,:]  = sum_k wf[i,k,:] @ weight[k]
"""
import torch

F64 = torch.float64


def influences(query, support, neighbors, k_points, extent):
    """w [n_q, K, n_nb] float64 and the clamped neighbour ids [n_q, n_nb]"""
    query, support, k_points = query.to(F64), support.to(F64), k_points.to(F64)
    n_s = support.shape[0]
    nb = neighbors.long()
    valid = (nb >= 0) & (nb < n_s)
    j = nb.clamp(0, max(n_s - 1, 0))
    rel = support[j] - query[:, None, :]                                   # [n_q, n_nb, 3]
    dist = (rel[:, None, :, :] - k_points[None, :, None, :]).pow(2).sum(-1).sqrt()   # [n_q, K, n_nb]
    w = (1.0 - dist / float(extent)).clamp(min=0.0) * valid[:, None, :].to(F64)
    return w, j


def kpconv_oracle(query, support, neighbors, x, k_points, weight, extent, add_one=False, return_wf=False, chunk=4096):
    """out [n_q, out] float64 (differentiable w.r.t. x and weight); all arguments CPU tensors of any float / int type"""
    x, weight = x.to(F64), weight.to(F64)
    if add_one:
        x = torch.cat([x, torch.ones_like(x[:, :1])], dim=1)
    n_q, n_s = query.shape[0], support.shape[0]
    n_kp, c, out = weight.shape
    if n_q == 0 or n_s == 0:
        wf = torch.zeros(n_q, n_kp, c, dtype=F64)
    else:
        parts = []
        for lo in range(0, n_q, chunk):
            w, j = influences(query[lo:lo + chunk], support, neighbors[lo:lo + chunk], k_points, extent)
            parts.append(w @ x[j])                                          # [q, K, n_nb] @ [q, n_nb, c]
        wf = torch.cat(parts)
    result = torch.einsum("qkc,kco->qo", wf, weight)
    return (result, wf) if return_wf else result
