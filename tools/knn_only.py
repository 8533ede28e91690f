"""The pass's kNN queries alone (diagnostic; GPU box only): k=16 of the n/4 sampled points among all, k=3 of all among the sampled."""
import sys
import torch
import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import scene, pointops as P
N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
xyz = torch.from_numpy(scene.make_room(N, 0)).cuda()
off = torch.tensor([N], dtype=torch.int32, device='cuda')
n4 = torch.tensor([N // 4 + 1], dtype=torch.int32, device='cuda')
idx = P.furthestsampling(xyz, off, n4).long()
sub = xyz[idx].contiguous()


def best_ms(fn, reps=5):
    return min(timing.calls([fn], reps, 0)[0][0])


print('N', N, 'k16 (%d queries in %d points) ms %.3f' % (sub.shape[0], N, best_ms(lambda: P.knnquery(16, xyz, sub, off, n4))),
      'k3 (%d queries in %d points) ms %.3f' % (N, sub.shape[0], best_ms(lambda: P.knnquery(3, sub, xyz, n4, off))))
