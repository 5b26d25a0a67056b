"""Float64 numpy statement of the grouped optimizer step (include/tld_hip.h: tld_opt_plan_create / tld_train_grad_guard_grouped /
tld_train_adamw_ema_grouped): the cut of the segments into chunks, the per-chunk, per-segment and global sums of squares in their stated
orders, the finalize rule with the schedule factor, and AdamW + EMA by group.  tests/test_opt_groups_host.py holds it against
torch.optim.AdamW + LambdaLR + clip_grad_norm_ in float64; tests/test_gpu_opt_groups.py holds the kernels against it.  As in
tests/grad_guard_ref.py nothing is rounded to fp32 except where the ABI or the kernel itself carries a float (``to_f32``)."""
import numpy as np

import grad_guard_ref as R

CHUNK = 8192                                  # OPT_CHUNK of csrc/tld_opt_plan.h
FACTOR = 7                                    # head index of the schedule factor


def cut(seg_numel):
    """The planner's cut: (first [n_chunks], length [n_chunks], segment [n_chunks], seg_chunk0 [n_seg + 1]) as int64 arrays."""
    seg_numel = np.asarray(seg_numel, dtype=np.int64)
    per = (seg_numel + CHUNK - 1) // CHUNK
    c0 = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    seg = np.repeat(np.arange(seg_numel.size, dtype=np.int64), per)
    start = np.concatenate([[0], np.cumsum(seg_numel)[:-1]]).astype(np.int64)
    within = np.arange(int(c0[-1]), dtype=np.int64) - c0[seg]
    first = start[seg] + within * CHUNK
    length = np.minimum(CHUNK, seg_numel[seg] - within * CHUNK)
    return first, length, seg, c0


def digest(seg_numel):
    """What tests/host/opt_plan_main.cpp prints for a segment list: (numel, n_chunks, chunk digest, range digest), the digests mod 2^64."""
    first, length, seg, c0 = (a.astype(np.uint64) for a in cut(seg_numel))
    with np.errstate(over="ignore"):
        idx = np.arange(first.size, dtype=np.uint64) + np.uint64(1)
        d_chunks = int((((first * np.uint64(1000003) + length) * np.uint64(31) + seg) * idx).sum(dtype=np.uint64))
        d_ranges = int((c0[:-1] * (np.arange(c0.size - 1, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64) + c0[-1])
    return int(np.sum(np.asarray(seg_numel, dtype=np.int64))), int(first.size), d_chunks, d_ranges


def segment_sqsums(g, scale, seg_numel):
    """seg[s]: the chunk sums of (g * float(scale))^2 added in chunk order."""
    first, length, seg, _ = cut(seg_numel)
    out = np.zeros(len(seg_numel), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for f, n, s in zip(first, length, seg):
            out[s] = out[s] + R.sqsum(g[f:f + n], scale)
    return out


def global_sqsum(seg_sq, seg_group, groups):
    """The segments whose group is not frozen, added in segment order."""
    tot = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for x, q in zip(seg_sq, seg_group):
            if not groups[q][2]:
                tot = tot + x
    return tot


def factor_at(table, t):
    return 1.0 if table is None or len(table) == 0 else float(table[min(int(t), len(table)) - 1])


def finalize(state, sumsq, max_norm, skip_nonfinite, b1, b2, table):
    """grad_guard_ref.finalize plus entry 7: the factor of the step count just reached; a skipped step keeps it."""
    keep = state[FACTOR]
    st = R.finalize(state, sumsq, max_norm, skip_nonfinite, b1, b2)
    st[FACTOR] = keep if st[R.LAST_SKIPPED] else factor_at(table, st[R.T])
    return st


def grouped_step(p, g, m, v, ema, state, seg_numel, seg_group, groups, table, lr, b1, b2, eps, alpha, scale=1.0, max_norm=None, skip_nonfinite=False,
                 to_f32=False):
    """One grouped step on float64 copies: returns (p, m, v, ema, state, seg_sq).  groups: [(lr_scale, weight_decay, frozen)].  to_f32: round the
    clip coefficient and the group's learning rate to float where the kernel does."""
    p, m, v = (np.array(a, dtype=np.float64) for a in (p, m, v))
    ema = None if ema is None else np.array(ema, dtype=np.float64)
    seg_sq = segment_sqsums(g, scale, seg_numel)
    st = finalize(state, global_sqsum(seg_sq, seg_group, groups), max_norm, skip_nonfinite, b1, b2, table)
    if st[R.LAST_SKIPPED]:
        return p, m, v, ema, st, seg_sq
    coef = R.f32(st[R.COEF]) if to_f32 else st[R.COEF]
    pos = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for n, q in zip(seg_numel, seg_group):
            sl = slice(pos, pos + int(n))
            pos += int(n)
            lr_scale, wd, frozen = groups[q]
            if frozen:
                continue
            lr_q = np.float64(lr) * np.float64(lr_scale) * st[FACTOR]
            if to_f32:
                lr_q = R.f32(lr_q)
            gi = (np.asarray(g[sl], dtype=np.float64) * np.float64(R.f32(scale))) * coef
            m[sl] = b1 * m[sl] + (1.0 - b1) * gi
            v[sl] = b2 * v[sl] + (1.0 - b2) * gi * gi
            ps = p[sl] * (1.0 - lr_q * wd)
            ps = ps - (lr_q / st[R.BC1]) * (m[sl] / (np.sqrt(v[sl]) / np.sqrt(st[R.BC2]) + eps))
            p[sl] = ps
            if ema is not None:
                ema[sl] = ema[sl] * alpha + ps * (1.0 - alpha)
    return p, m, v, ema, st, seg_sq
