#!/usr/bin/env python
"""sha256 of everything a differentiable rollout computes, for comparing two
trees bit by bit (a -0 / +0 flip included, which torch.equal does not see).

  python scripts/rollout_refactor_sha256.py TREE_ROOT > listing.txt
Imports the package and the test helpers of TREE_ROOT (which must be built) and
prints one line per run, with the digest of each ``out`` and ``observed.grad`` and
one digest over the "name digest" lines of every BatchNorm buffer and one over
those of every parameter's gradient, of DSTDGCN.rollout and rollout_pair, train mode,
dropout off, fixed seeds, through autograd's arenas and in place, for the three
families of entry points -- whole windows, whole windows with a teacher, and a
stride (free running and with a teacher) -- on the SMALL cases of
tests/test_gpu_rollout.py, test_gpu_teacher.py and test_gpu_rollout_stride.py
and on the h36m model at B = 2.  Two trees compute the same when their listings
are equal (profiles/rollout_refactor_sha256.txt holds the parent's and this
tree's side by side).
"""
import hashlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(ROOT, "dstd-gcn_amd"), os.path.join(ROOT, "tests"), ROOT]
import torch  # noqa: E402
import test_gpu_rollout as plain  # noqa: E402
import test_gpu_rollout_stride as strided  # noqa: E402
import test_gpu_teacher as teacher  # noqa: E402

B = 2


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def runs():
    """(tag, model, Tin, V, stride, horizon, masked) of every case"""
    for case in plain.CASES:
        m, _, Tin, V, H = plain.case_model(case)
        yield f"plain {case}", m, Tin, V, None, H, False
    for case in teacher.CASES + ["h36m"]:
        m, Tin, V, H = teacher.case_model(case)
        yield f"teacher {case}", m, Tin, V, None, H, True
    for case in strided.CASES + ["h36m"]:
        for masked in (False, True):
            m, Tin, V, S, H = strided.case_model(case)
            yield f"strided-{'teacher' if masked else 'free'} {case}", m, Tin, V, S, H, masked


def main():
    for tag, model, Tin, V, S, H, masked in runs():
        K = -(-H // (S or model.output_time_frame))
        state = {k: v.clone() for k, v in model.state_dict().items()}
        truth = plain.observations(B, Tin + H, V, 7)
        for pair in (False, True):
            tf = dict(teacher=truth, teacher_mask=strided.mask_of("mixed", K, 2 * B if pair else B, pair)) if masked else {}
            for inplace in (False, True):
                model.load_state_dict(state)
                model.train()
                model.do_in.p = 0.0
                model._dstd_inplace_grads = inplace
                model.zero_grad(set_to_none=True)
                obs = [plain.observations(B, Tin, V, 11 + i).requires_grad_() for i in range(2 if pair else 1)]
                outs = model.rollout_pair(*obs, H, stride=S, **tf) if pair else (model.rollout(obs[0], H, stride=S, **tf),)
                (sum(o.square().sum() for o in outs) / outs[0].numel()).backward()
                torch.cuda.synchronize()
                run = f"{tag} {'rollout_pair' if pair else 'rollout'} {'inplace' if inplace else 'autograd'}"
                cols = [(f"out{i}", sha(o)) for i, o in enumerate(outs)] + [(f"dobs{i}", sha(o.grad)) for i, o in enumerate(obs)]
                grads = [(k, p.grad) for k, p in model.named_parameters() if p.grad is not None]
                for what, named in (("buffers", list(model.named_buffers())), ("grads", grads)):
                    each = "".join(f"{k} {sha(t)}\n" for k, t in named)
                    cols.append((f"{what}[{len(named)}]", hashlib.sha256(each.encode()).hexdigest()))
                print(f"{run} | " + " ".join(f"{k} {v}" for k, v in cols))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
