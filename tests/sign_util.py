"""Shared by tests/test_sign_majority.py and tests/test_sign_majority_gpu.py: the input
family and the plain int64 statement of the majority vote."""
import torch

SUB = 2.0 ** -140  # an fp32 subnormal
FAMILY = torch.tensor([1.5, -2.25, 3e-5, -7.0, 0.0, -0.0, float("nan"), float("inf"),
                       float("-inf"), SUB, -SUB])
ABSTAIN = torch.tensor([0.0, -0.0, float("nan")])


def sign_case(P, n, seed):
    """(P, n) from FAMILY; column 0 unanimous, 1 all-abstain, 2 a tie of rows 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    x = FAMILY[torch.randint(len(FAMILY), (P, n), generator=g)]
    x[:, 0] = -SUB
    x[:, 1] = x[:, 2] = ABSTAIN[torch.arange(P) % 3]
    x[:2, 2] = torch.tensor([float("inf"), -3.0])[:P]
    return x


def sign_ref(x):
    """(votes, out): votes = sign(x) with NaN -> 0 as int64, out = sign(votes.sum(0))."""
    votes = torch.nan_to_num(torch.sign(x), nan=0.0).to(torch.int64)
    return votes, torch.sign(votes.sum(0)).float()


def pack_rows(ops, x):
    out = torch.empty(x.shape[0], x.shape[1] // 16, dtype=torch.int32, device=x.device)
    for p in range(x.shape[0]):
        ops.sign_pack(x[p], out[p])
    return out


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
