"""Drop-in for python/fate_llm/algo/fedkseed/zo_utils.py (FATE-LLM 2.2.0).

``directional_derivative_step`` (reference :23-54) runs on the MI355X codec;
``reconstruct_`` is the batched form ClientTrainer.train_once uses (one device pass
for all K seeds instead of K Python-level passes).  The scalar helpers
(``probability_from_amps`` :6-20, ``build_seed_candidates`` :57-61,
``get_even_seed_probabilities`` :64-68) operate on K-sized vectors and stay in torch.
"""
from typing import List, Sequence

import numpy as np
import torch

from . import codec


def probability_from_amps(amps: List[List[float]], clip):
    """Seed-sampling distribution from each seed's directional-derivative history.

    amp_i = mean(|clamp(history_i, -clip, clip)|), min-max normalised, then softmax.
    Same arithmetic as the reference (fp32 torch ops, +1e-10 in the denominator).
    """
    per_seed = []
    for history in amps:
        h = torch.tensor(history, dtype=torch.float32)
        per_seed.append(h.clamp(-clip, clip).abs().mean())
    amp = torch.stack(per_seed)
    lo, hi = amp.min(), amp.max()
    return ((amp - lo) / (hi - lo + 1e-10)).softmax(0)


def _value_kind(value, specs=(), stream_mode=None):
    """(g as a python float, whether it is a tensor): a tensor g is cast to each
    parameter's dtype by the reference's ``g * z`` (zo_utils.py:49).  A 1-element tensor
    that is not 0-dim takes part in type promotion and broadcasting as a dimensioned
    tensor: that is the same update when the promoted dtype is the parameter's own and
    the parameter has a dimension; otherwise the reference rebinds ``param.data`` to a
    tensor of another dtype or shape, which an in-place update cannot be -- raised.

    Where z lives decides the cast: on the CPU (the torch_cpu stream) TensorIterator
    promotes the 0-dim g to the parameter dtype before the f32 multiply; with z on a GPU
    (the torch_rocm stream) a 0-dim g on the GPU is cast the same way (the kernel's
    dynamic-cast load), but a 0-dim g on the CPU is a "CPU scalar" whose f32 value enters
    the kernel unrounded (gpu_kernel_with_scalars: scalar_value<opmath_t>) -- the same
    multiply as a python number -- and a dimensioned CPU g is torch's device-mismatch
    error."""
    if isinstance(value, torch.Tensor) and value.device.type == "cpu" and specs:
        dev = specs[0].tensor.device
        if dev.type == "cuda" and codec.resolve_stream_mode(dev, stream_mode) == "torch_rocm":
            if value.dim() != 0:
                raise RuntimeError("Expected all tensors to be on the same device, but found at least two devices, "
                                   f"{dev} and cpu! (a {tuple(value.shape)} directional_derivative_value on the CPU "
                                   "times z on the GPU, zo_utils.py:49)")
            return float(value.item()), False
    if isinstance(value, torch.Tensor):
        if value.dim() != 0:
            if value.numel() != 1:
                raise ValueError("directional_derivative_value must be a python number or a 1-element tensor")
            for sp in specs:
                t = sp.tensor
                if torch.promote_types(value.dtype, t.dtype) != t.dtype or t.dim() == 0:
                    raise NotImplementedError(
                        f"a {tuple(value.shape)} {value.dtype} directional_derivative_value would turn a "
                        f"{tuple(t.shape)} {t.dtype} parameter into {torch.promote_types(value.dtype, t.dtype)} "
                        "of the broadcast shape (the reference rebinds param.data); pass a 0-dim tensor")
        return float(value.reshape(()).item()), True
    return float(value), False


def directional_derivative_step(
    param_groups: List[dict],
    directional_derivative_seed: int,
    directional_derivative_value: torch.FloatTensor,
    lr: float = None,
    weight_decay: float = None,
) -> torch.FloatTensor:
    """p <- p - lr * (value * z + weight_decay * p) along z = N(0, 1) drawn from
    ``directional_derivative_seed``, for every parameter of every group in order
    (or p <- p - lr * value * z when the resolved weight_decay is None).

    lr / weight_decay default to the first group's values and then stick for every
    later group, exactly as the reference resolves them.  Parameters are updated in
    place on the GPU, and torch's generators are left where the reference's
    torch.manual_seed and draws leave them (the generator of the parameters' device past
    this seed's z).
    """
    torch.manual_seed(directional_derivative_seed)
    specs = codec.resolve_groups(param_groups, lr=lr, weight_decay=weight_decay)
    v, is_tensor = _value_kind(directional_derivative_value, specs)
    codec.directional_step(specs, [directional_derivative_seed], [v], value_is_tensor=is_tensor)
    codec.mark_rebound(p for g in param_groups for p in g["params"])  # zo_utils.py:49 rebinds param.data
    return directional_derivative_value


def reconstruct_(param_groups: List[dict], seeds: Sequence[int], values: Sequence[float], lr: float,
                 weight_decay: float) -> int:
    """The reconstruct loop of ClientTrainer.train_once (fedkseed.py:136-141) in one pass:
    for (seed, value) in order, skip exact zeros (NaN is applied, as in the reference),
    then directional_derivative_step(param_groups, seed, value, lr=lr, weight_decay=weight_decay).
    Returns the number of seeds applied."""
    keep = [(int(s), float(g)) for s, g in zip(seeds, values) if float(g) != 0.0]
    if not keep:
        return 0
    specs = codec.resolve_groups(param_groups, lr=lr, weight_decay=weight_decay)
    # the same list comes back every round (the arbiter's fixed seed candidates): keep the
    # jumped generator windows for the next reconstruct (codec.jwin_reserve, a speed cache).
    # torch's generators end where the last applied seed's draws leave them (codec._leave).
    codec.directional_step(specs, [s for s, _ in keep], [g for _, g in keep], value_is_tensor=False,
                           cache_windows=True)
    codec.mark_rebound(p for g in param_groups for p in g["params"])
    return len(keep)


def seed_shard_coefficients(values: Sequence[float], lr: float, weight_decay, rank: int = 0, world: int = 1):
    """Seed-sharded variant (BASELINE config C3): the K sequential steps
    p <- p - lr*(g_k*z_k + wd*p) of the reconstruct sum to
    p_K = a^K p_0 - sum_k lr g_k a^(K-1-k) z_k with a = 1 - lr*wd (a = 1 without the
    decay term).  Returns (first, last) -- the seed index range [first, last) rank
    ``rank`` of ``world`` accumulates, a contiguous 1/world of the K seeds -- the
    coefficients lr g_k a^(K-1-k) of that range (float64), and a^K.
    lr and wd enter as the fp32 values the reference's opmath sees."""
    import math

    import numpy as np

    k = len(values)
    first, last = k * rank // world, k * (rank + 1) // world
    lr32 = float(np.float32(lr))
    if weight_decay is None:
        log_a = 0.0
    else:
        log_a = math.log1p(-lr32 * float(np.float32(weight_decay)))
    coefs = [lr32 * float(values[i]) * math.exp((k - 1 - i) * log_a) for i in range(first, last)]
    return first, last, coefs, math.exp(k * log_a)


def reconstruct_seed_sharded_(param_groups: List[dict], seeds: Sequence[int], values: Sequence[float], lr: float,
                              weight_decay: float, process_group=None, delta: torch.Tensor = None) -> int:
    """The reconstruct of ClientTrainer.train_once as the north star's seed-sharded
    variant: every rank of ``process_group`` (torch.distributed, RCCL on MI355X) takes a
    contiguous 1/world of the non-zero seeds, accumulates its part of the f32 delta on
    its GPU, one all-reduce sums the parts, and every rank applies p = a^K p_0 - delta.

    NOT bit-equal to ``reconstruct_`` / the reference (which rounds every op of every
    seed to the parameter dtype): see DESIGN.md §7 for the measured deviation.  All
    tensors must share one (lr, wd) -- train_once passes them explicitly, so the sticky
    rule makes them uniform.  ``delta``: optional preallocated f32 buffer (the
    parameters' concatenation), zeroed here.  Returns the number of seeds applied."""
    import torch.distributed as dist

    keep = [(int(s), float(g)) for s, g in zip(seeds, values) if float(g) != 0.0]
    if not keep:
        return 0
    specs = codec.resolve_groups(param_groups, lr=lr, weight_decay=weight_decay)
    classes = {(sp.lr, sp.weight_decay) for sp in specs}
    if len(classes) != 1:
        raise ValueError("seed-sharded reconstruct needs one (lr, weight_decay) for every tensor")
    distributed = process_group is not None or (dist.is_available() and dist.is_initialized())
    rank = dist.get_rank(process_group) if distributed else 0
    world = dist.get_world_size(process_group) if distributed else 1
    sp0 = specs[0]
    first, last, coefs, decay = seed_shard_coefficients([g for _, g in keep], sp0.lr, sp0.weight_decay, rank, world)
    total = sum(sp.tensor.numel() for sp in specs)
    dev = sp0.tensor.device
    if delta is None:
        delta = torch.zeros(total, dtype=torch.float32, device=dev)
    else:
        delta.zero_()
    codec.delta_accumulate(specs, [s for s, _ in keep[first:last]], coefs, delta)
    if distributed:  # also at world size 1: the group's collective library sums (an identity)
        dist.all_reduce(delta, op=dist.ReduceOp.SUM, group=process_group)
    codec.delta_apply(specs, delta, [decay] * len(specs))
    codec.leave_generators(specs, keep[-1][0])  # where the reference's last seed leaves them
    return len(keep)


def _projection_inputs(param_groups: List[dict], vectors):
    """(specs, vec, N): the parameters of every group in the codec's order -- one that does
    not require grad is frozen: it draws its z and contributes nothing --, the vectors
    flattened into the f32 concatenation codec.project reads (a frozen parameter's range is
    zero), and the number of non-frozen elements."""
    params = [p for g in param_groups for p in g["params"]]
    if vectors is None:
        vectors = [p.grad if p.requires_grad else None for p in params]
    vectors = list(vectors)
    if len(vectors) != len(params):
        raise ValueError(f"one vector per parameter: {len(params)} parameters, {len(vectors)} vectors")
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    if not params:
        return specs, None, 0
    total = sum(p.numel() for p in params)
    vec = torch.empty(total, dtype=torch.float32, device=params[0].device)
    at = n_live = 0
    for i, (p, v) in enumerate(zip(params, vectors)):
        dst = vec[at:at + p.numel()]
        at += p.numel()
        if not p.requires_grad:
            dst.zero_()
            continue
        if v is None:
            raise ValueError(f"parameter {i} requires grad and has no vector (its .grad is None)")
        if not v.is_floating_point() or v.numel() != p.numel():
            raise ValueError(f"vector {i}: a floating-point tensor of {p.numel()} elements is needed, "
                             f"got {v.dtype} {tuple(v.shape)}")
        dst.copy_(v.detach().reshape(-1))
        n_live += p.numel()
    return specs, vec, n_live


def _project_on_stream(specs, seeds, vec, stream_mode):
    """codec.project on the torch_rocm stream, codec.project_mt on torch_cpu: the stream the
    call resolves to on the vector's device."""
    if codec.resolve_stream_mode(vec.device, stream_mode) == "torch_cpu":
        return codec.project_mt(specs, seeds, vec)
    return codec.project(specs, seeds, vec, stream_mode=stream_mode)


def seed_projections(param_groups: List[dict], seeds: Sequence[int], vectors=None, stream_mode=None) -> torch.Tensor:
    """g_k = <v, z_k> for every seed: the exact directional derivatives of the K seed
    candidates along a dense vector -- with v the gradient, one backward pass instead of two
    forward passes per seed, and no finite-difference noise; the K scalars the wire carries.

    ``vectors``: one tensor per parameter of the groups, in order, of any float dtype (the
    entry of a parameter that does not require grad is ignored and may be None); default:
    every parameter's ``.grad`` (a missing grad on a parameter that requires grad is an
    error).  z_k is the stream ``directional_derivative_step`` draws for seed k: every
    parameter draws, in each one's own dtype; those that do not require grad contribute
    nothing.  Mind the consequence: ``directional_derivative_step`` itself freezes nothing
    -- like the reference's, it updates every parameter of the groups, whatever its
    ``requires_grad`` -- so the K values are the exact derivatives of the step it applies
    only when every parameter of the groups requires grad (the groups
    ``pytorch_utils.get_optimizer_parameters_grouped_with_decay`` builds hold only such
    parameters); with a parameter that does not, the step moves it along z as well and its
    term is missing here.
    The vectors are read as f32, and each call lays them out in a new f32 buffer of the
    model's size, so its first launch also builds the buffer's tensor table (an allocation and
    a synchronous upload; codec.project).  Returns float64[K] on the parameters' device,
    queued on the current stream (exact products, f64 sums, bit-reproducible), on either stream:
    a call that resolves to torch_rocm takes codec.project, one that resolves to torch_cpu
    codec.project_mt.  torch's generators are left alone.
    ``seed_projections_multi`` reads the vectors in place, in their own dtype, several per pass
    (torch_rocm stream only)."""
    specs, vec, _ = _projection_inputs(param_groups, vectors)
    if vec is None:
        return torch.zeros(len(seeds), dtype=torch.float64)
    return _project_on_stream(specs, seeds, vec, stream_mode)


def fit_seed_scalars(param_groups: List[dict], seeds: Sequence[int], delta_vectors, stream_mode=None) -> torch.Tensor:
    """The (seed, scalar) form of a dense update: ``seed_projections(delta) / N``, N the
    number of elements of the parameters that require grad -- how a fine-tuned checkpoint's
    or a FedAvg round's delta enters a running federation.

    An approximation: the least-squares scalars in the candidates' span are
    (Z^T Z)^-1 Z^T delta, and the Gram matrix Z^T Z equals N I only in expectation -- its
    diagonal deviates from N by O(sqrt(2 N)), its off-diagonal entries are O(sqrt(N)) --, so
    these scalars differ from the least-squares ones by a relative error of order
    sqrt(K / N): negligible for K << N.  What is fitted is the projection of delta on the
    K-seed subspace, a share of about K / N of a generic delta's energy.  Either stream, as
    ``seed_projections``.
    ``fit_seed_scalars_multi`` fits several deltas in one pass, each read in place (torch_rocm only).
    ``fit_seed_scalars_exact`` solves with the Gram matrix itself and has no sqrt(K / N) error."""
    specs, vec, n_live = _projection_inputs(param_groups, delta_vectors)
    if vec is None or n_live == 0:
        raise ValueError("fit_seed_scalars: no parameter requires grad")
    return _project_on_stream(specs, seeds, vec, stream_mode) / float(n_live)


def _projection_specs(param_groups: List[dict], vector_lists):
    """(specs, vector lists, N) of the in-place forms: no buffer is built, codec.project_multi
    reads every tensor where it lies."""
    params = [p for g in param_groups for p in g["params"]]
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    if vector_lists is None:
        for i, p in enumerate(params):
            if p.requires_grad and p.grad is None:
                raise ValueError(f"parameter {i} requires grad and has no vector (its .grad is None)")
        vector_lists = [[p.grad if p.requires_grad else None for p in params]]
    vector_lists = [list(vs) for vs in vector_lists]
    for m, vs in enumerate(vector_lists):
        if len(vs) != len(params):
            raise ValueError(f"vector list {m}: one vector per parameter: {len(params)} parameters, {len(vs)} vectors")
    return specs, vector_lists, sum(p.numel() for p in params if p.requires_grad)


def seed_projections_multi(param_groups: List[dict], seeds: Sequence[int], vector_lists=None,
                           stream_mode=None) -> torch.Tensor:
    """``seed_projections`` of M vector lists in one call, float64[M, K]: every vector is read
    where it lies, in its own dtype (a bf16 model's ``.grad``s as bf16: no f32 buffer of the
    model's size, no conversion pass), and up to four lists share each pass of the generator
    (codec.project_multi).  ``vector_lists``: M lists with one tensor per parameter (None for
    a parameter that does not require grad); default: one list, every parameter's ``.grad``,
    and a [1, K] result.  Row m equals the one-list call on list m bit for bit, and equals
    ``seed_projections`` of the same vectors bit for bit.  torch_rocm stream only: a call that
    resolves to torch_cpu raises; ``seed_projections_in_place`` takes either stream."""
    specs, vector_lists, _ = _projection_specs(param_groups, vector_lists)
    if not specs:
        return torch.zeros((len(vector_lists), len(seeds)), dtype=torch.float64)
    return codec.project_multi(specs, seeds, vector_lists, stream_mode=stream_mode)


def fit_seed_scalars_multi(param_groups: List[dict], seeds: Sequence[int], delta_vector_lists,
                           stream_mode=None) -> torch.Tensor:
    """``fit_seed_scalars`` of M dense deltas in one call: ``seed_projections_multi / N``,
    float64[M, K] -- an arbiter turning the deltas of several first-order or FedAvg parties
    into (seed, scalar) form pays for one pass of the generator per four parties.  torch_rocm
    stream only; ``fit_seed_scalars_in_place`` takes either stream.  ``fit_seed_scalars_exact`` is the
    exact least-squares form (no sqrt(K / N) error)."""
    specs, vector_lists, n_live = _projection_specs(param_groups, delta_vector_lists)
    if not specs or n_live == 0:
        raise ValueError("fit_seed_scalars_multi: no parameter requires grad")
    return codec.project_multi(specs, seeds, vector_lists, stream_mode=stream_mode) / float(n_live)


def _project_in_place_on_stream(specs, seeds, vector_lists, stream_mode):
    """codec.project_multi on the torch_rocm stream, codec.project_mt_multi on torch_cpu: the
    stream the call resolves to on the parameters' device."""
    if codec.resolve_stream_mode(specs[0].tensor.device, stream_mode) == "torch_cpu":
        return codec.project_mt_multi(specs, seeds, vector_lists)
    return codec.project_multi(specs, seeds, vector_lists, stream_mode=stream_mode)


def seed_projections_in_place(param_groups: List[dict], seeds: Sequence[int], vector_lists=None,
                              stream_mode=None) -> torch.Tensor:
    """``seed_projections_multi`` on either stream, float64[M, K]: a call that resolves to
    torch_rocm takes codec.project_multi, one that resolves to torch_cpu codec.project_mt_multi.
    Every vector is read where it lies, in its own dtype -- no f32 buffer of the model's size, no
    conversion pass, no plan keyed on a buffer's address -- and up to four lists (torch_rocm) or
    two (torch_cpu) share each pass of the generator.  ``vector_lists`` and the default (one list, every parameter's ``.grad``,
    a [1, K] result; a missing grad on a parameter that requires grad is an error) are
    ``seed_projections_multi``'s.  Row m equals the one-list call on list m bit for bit, and
    equals ``seed_projections`` of the same vectors on the same stream bit for bit.  torch's
    generators are left alone."""
    specs, vector_lists, _ = _projection_specs(param_groups, vector_lists)
    if not specs:
        return torch.zeros((len(vector_lists), len(seeds)), dtype=torch.float64)
    return _project_in_place_on_stream(specs, seeds, vector_lists, stream_mode)


def fit_seed_scalars_in_place(param_groups: List[dict], seeds: Sequence[int], delta_vector_lists,
                              stream_mode=None) -> torch.Tensor:
    """``fit_seed_scalars_multi`` on either stream: ``seed_projections_in_place / N``,
    float64[M, K], through codec.project_multi (torch_rocm) or codec.project_mt_multi
    (torch_cpu).  ``fit_seed_scalars_exact`` is the exact least-squares form (no sqrt(K / N) error)."""
    specs, vector_lists, n_live = _projection_specs(param_groups, delta_vector_lists)
    if not specs or n_live == 0:
        raise ValueError("fit_seed_scalars_in_place: no parameter requires grad")
    return _project_in_place_on_stream(specs, seeds, vector_lists, stream_mode) / float(n_live)


def seed_gram(param_groups: List[dict], seeds: Sequence[int], col_seeds=None, stream_mode=None) -> torch.Tensor:
    """The Gram matrix of the seed basis over the groups' parameters, G[r, c] = <z_r, z_c>
    (codec.gram): float64[K, K] for ``seeds`` alone (Z^T Z, exactly symmetric), float64[Kr, Kc]
    with ``col_seeds``.  z_k is the stream ``seed_projections`` uses: every parameter draws, in
    its own dtype, and one that does not require grad is frozen -- it draws and contributes
    nothing --, so G is the Gram matrix of exactly the vectors ``seed_projections_in_place``
    projects on, and its diagonal holds their exact squared norms |z_k|^2.  Nothing of the
    model's size is allocated.  Queued on the current stream; torch's generators are left alone.
    torch_rocm stream only; ``seed_gram_on_stream`` takes either stream."""
    params = [p for g in param_groups for p in g["params"]]
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    return codec.gram(specs, seeds, col_seeds, stream_mode=stream_mode)


def _solve_normal_equations(G, b):
    """x with G x[m] = b[m] for every row m of b (float64[M, K]; G float64[K, K], symmetric
    positive definite), by Cholesky in float64 on the host: G = L L^T, then the two triangular
    systems.  A G that is not positive definite raises ValueError."""
    G = np.asarray(G, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    try:
        low = np.linalg.cholesky(G)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the seeds' Gram matrix ({G.shape[0]} x {G.shape[0]}) is not positive definite: the z of "
                         "the seeds are linearly dependent over the parameters that require grad (more seeds than "
                         "such elements, or a repeated seed)") from e
    y = np.linalg.solve(low, b.T)
    return np.linalg.solve(low.T, y).T


def _fit_exact(name, param_groups, seeds, delta_vector_lists, stream_mode, on_stream, tiled=False):
    """fit_seed_scalars_exact (on_stream False: torch_rocm only),
    fit_seed_scalars_exact_on_stream (True: either stream) and fit_seed_scalars_exact_tiled
    (tiled True: torch_rocm only, G through codec.gram_tiled): the duplicate-seed check,
    b = Z^T delta read in place, G = Z^T Z on the same stream, the host solve.  SYNCHRONISES: G
    and b are copied to the host."""
    seen = set()
    for s in seeds:
        if int(s) in seen:
            raise ValueError(f"{name}: seed {int(s)} is given twice; the scalars of a repeated seed "
                             "are not unique")
        seen.add(int(s))
    specs, vector_lists, n_live = _projection_specs(param_groups, delta_vector_lists)
    if not specs or n_live == 0:
        raise ValueError(f"{name}: no parameter requires grad")
    mode = codec.resolve_stream_mode(specs[0].tensor.device, stream_mode)
    if mode != "torch_rocm" and not on_stream:  # before the projection, which has a torch_cpu form, runs for nothing
        raise NotImplementedError(f"{name}: the Gram matrix is built for the torch_rocm stream only here; "
                                  f"this call resolves to the {mode} stream (fit_seed_scalars_exact_on_stream takes "
                                  "either stream)")
    b = _project_in_place_on_stream(specs, seeds, vector_lists, stream_mode)
    if tiled:
        G = codec.gram_tiled(specs, seeds, stream_mode=stream_mode)
    else:
        G = codec.gram_mt(specs, seeds) if mode == "torch_cpu" else codec.gram(specs, seeds, stream_mode=stream_mode)
    x = _solve_normal_equations(G.cpu().numpy(), b.cpu().numpy())
    return torch.from_numpy(np.ascontiguousarray(x)).to(b.device)


def fit_seed_scalars_exact(param_groups: List[dict], seeds: Sequence[int], delta_vector_lists,
                           stream_mode=None) -> torch.Tensor:
    """The exact least-squares form of ``fit_seed_scalars_in_place``: the scalars
    (Z^T Z)^-1 Z^T delta that minimise |delta - Z c|_2 for each of the M dense deltas,
    float64[M, K] on the parameters' device.  b = ``seed_projections_in_place`` (Z^T delta, every
    delta read where it lies) and G = ``seed_gram`` (Z^T Z) come from the device, both exact up
    to f64 summation; the K x K system is solved on the host in float64 by Cholesky
    (``_solve_normal_equations``).  Where ``fit_seed_scalars*`` err by a relative sqrt(K / N) --
    3 % for an adapter of 4M elements at K = 4096, 10 % for a head of 3,000 at K = 40 -- this
    is exact: a delta that lies in the seeds' span is recovered to the precision it was stored
    in.  The call SYNCHRONISES: G and b are copied to the host.  Duplicate seeds raise
    ValueError (their columns of Z coincide and the scalars are not unique), and so does a G
    that is not positive definite: more seeds than elements that require grad.  torch_rocm
    stream only, as ``seed_gram``; ``fit_seed_scalars_exact_on_stream`` takes either stream."""
    return _fit_exact("fit_seed_scalars_exact", param_groups, seeds, delta_vector_lists, stream_mode, False)


def seed_gram_tiled(param_groups: List[dict], seeds: Sequence[int], col_seeds=None, stream_mode=None) -> torch.Tensor:
    """``seed_gram`` through codec.gram_tiled: the same matrix, G[r, c] = <z_r, z_c> over the
    parameters that require grad, in passes of 64 x 64 seeds on the f64 matrix unit -- the form for
    seed counts in the hundreds and thousands, where ``seed_gram``'s passes of 4 x 32 seeds are too
    many.  Arguments and meaning are ``seed_gram``'s; the products are exact and the sums f64 in
    a fixed order of the tiled kernel's own, so G is exactly symmetric and reproducible but agrees
    with ``seed_gram`` to within 2 n 2^-52 sum|z_r z_c| only, not bit for bit.  torch_rocm stream
    only; ``seed_gram`` and ``seed_gram_on_stream`` keep their bits and their routing."""
    params = [p for g in param_groups for p in g["params"]]
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    return codec.gram_tiled(specs, seeds, col_seeds, stream_mode=stream_mode)


def fit_seed_scalars_exact_tiled(param_groups: List[dict], seeds: Sequence[int], delta_vector_lists,
                                 stream_mode=None) -> torch.Tensor:
    """``fit_seed_scalars_exact`` with G from ``seed_gram_tiled``: the least-squares scalars
    (Z^T Z)^-1 Z^T delta, float64[M, K], where K is large enough that G is the cost of the fit.
    b, the host solve, the errors (a repeated seed, a G that is not positive definite) and the
    synchronisation are ``fit_seed_scalars_exact``'s; the scalars differ from its by the f64
    summation order of G only.  torch_rocm stream only."""
    return _fit_exact("fit_seed_scalars_exact_tiled", param_groups, seeds, delta_vector_lists, stream_mode, False,
                      tiled=True)


def seed_gram_on_stream(param_groups: List[dict], seeds: Sequence[int], col_seeds=None, stream_mode=None) -> torch.Tensor:
    """``seed_gram`` on either stream: a call that resolves to torch_rocm takes codec.gram, one
    that resolves to torch_cpu codec.gram_mt (the precedent is ``seed_expansion_on_stream_``).
    Arguments and result are ``seed_gram``'s; on torch_rocm the bits are ``seed_gram``'s too.  On
    torch_cpu G is the Gram matrix of the CPU generator's draws -- the stream of a federation
    whose reference clients train on the CPU --: its diagonal holds the exact |z_k|^2, and with
    ``seed_projections_in_place`` it gives the share of a gradient the seed span captures."""
    params = [p for g in param_groups for p in g["params"]]
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    device = specs[0].tensor.device if specs else torch.device("cpu")
    if codec.resolve_stream_mode(device, stream_mode) == "torch_cpu":
        return codec.gram_mt(specs, seeds, col_seeds)
    return codec.gram(specs, seeds, col_seeds, stream_mode=stream_mode)


def fit_seed_scalars_exact_on_stream(param_groups: List[dict], seeds: Sequence[int], delta_vector_lists,
                                     stream_mode=None) -> torch.Tensor:
    """``fit_seed_scalars_exact`` on either stream: b through codec.project_multi and G through
    codec.gram on torch_rocm (``fit_seed_scalars_exact``'s bits), through codec.project_mt_multi
    and codec.gram_mt on torch_cpu -- so a dense delta enters a federation on the CPU generator's
    stream without the sqrt(K / N) error of ``fit_seed_scalars_in_place``.  Arguments, result and
    errors (a repeated seed, a Gram matrix that is not positive definite) are
    ``fit_seed_scalars_exact``'s.  The call SYNCHRONISES: G and b are copied to the host."""
    return _fit_exact("fit_seed_scalars_exact_on_stream", param_groups, seeds, delta_vector_lists, stream_mode, True)


def _expansion_outputs(params, outputs, m=None):
    """One output list for ``params``: the given tensors (the entry of a parameter that does not
    require grad is dropped), or by default every parameter's ``.grad``, created as zeros in the
    parameter's dtype where it is None."""
    where = "" if m is None else f"output list {m}: "
    if outputs is None:
        outs = []
        for p in params:
            if not p.requires_grad:
                outs.append(None)
                continue
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            outs.append(p.grad)
        return outs
    outputs = list(outputs)
    if len(outputs) != len(params):
        raise ValueError(f"{where}one output per parameter: {len(params)} parameters, {len(outputs)} outputs")
    return [o if p.requires_grad else None for p, o in zip(params, outputs)]


def seed_expansions_(param_groups: List[dict], seeds: Sequence[int], scalar_lists, output_lists,
                     accumulate: bool = False, stream_mode=None):
    """``seed_expansion_`` for M outputs in one call: output_lists[m] = (or += with
    ``accumulate``) sum_k scalar_lists[m][k] z_k.  The z of a seed are drawn once for up to four
    outputs (codec.expand_multi); row m equals the single call bit for bit.  An entry of
    ``output_lists`` may be None for the default (every parameter's ``.grad``).  Returns the list
    of output lists."""
    params = [p for g in param_groups for p in g["params"]]
    scalar_lists = [list(c) for c in scalar_lists]
    output_lists = list(output_lists)
    if len(scalar_lists) != len(output_lists):
        raise ValueError(f"one scalar list per output list: {len(output_lists)} output lists, "
                         f"{len(scalar_lists)} scalar lists")
    outs = [_expansion_outputs(params, o, m) for m, o in enumerate(output_lists)]
    if not params or not outs:
        return outs
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    betas = [1.0 if accumulate else 0.0] * len(outs)
    detached = [[None if o is None else o.detach() for o in os_] for os_ in outs]
    codec.expand_multi(specs, seeds, scalar_lists, detached, betas=betas, stream_mode=stream_mode)
    return outs


def seed_expansion_(param_groups: List[dict], seeds: Sequence[int], scalars: Sequence[float], outputs=None,
                    accumulate: bool = False, stream_mode=None):
    """The dense vector of (seed, scalar) pairs, sum_k scalars[k] z_k, written (or added, with
    ``accumulate``) into ``outputs`` -- the other direction of ``seed_projections``: what
    ``fit_seed_scalars*`` made of a dense delta, handed back as dense tensors; the zeroth-order
    gradient estimate sum_k g_k z_k where a torch optimizer looks for it; the Z c of the residual
    delta - Z c that shows how well a fit holds.

    ``outputs``: one contiguous float32 / bfloat16 / float16 tensor per parameter of the groups,
    in order, each with its parameter's element count and on its device, of any of the three
    dtypes (the entry of a parameter that does not require grad is ignored and may be None);
    default: every parameter's ``.grad``, created in the parameter's dtype where it is None -- so
    ``torch.optim.AdamW(...).step()``, gradient clipping or accumulation follow as after a
    backward pass.  z_k is the stream ``directional_derivative_step`` draws for seed k: every
    parameter draws in its own dtype; those that do not require grad are frozen (drawn, not
    written).  The sum is an f32 fma chain in seed order held in registers over all the seeds and
    rounded once to the output's dtype (codec.expand_multi): no f32 buffer of the model's size
    and no pass over memory per 32 seeds.  Queued on the current stream; torch's generators are
    left alone.  torch_rocm stream only: a call that resolves to torch_cpu raises
    NotImplementedError (``seed_expansion_on_stream_`` takes either stream).  Returns the list of
    outputs."""
    return seed_expansions_(param_groups, seeds, [list(scalars)], [outputs], accumulate=accumulate,
                            stream_mode=stream_mode)[0]


def seed_expansions_on_stream_(param_groups: List[dict], seeds: Sequence[int], scalar_lists, output_lists,
                               accumulate: bool = False, stream_mode=None):
    """``seed_expansions_`` on either stream: a call that resolves to torch_rocm takes
    codec.expand_multi, one that resolves to torch_cpu codec.expand_mt_multi (the precedent is
    ``seed_projections_in_place``).  Arguments, defaults (``.grad``, created in the parameter's
    dtype where it is None; ``accumulate``) and the result are ``seed_expansions_``'s.  On
    torch_cpu up to 19 seeds are one pass with the sums in registers -- the zeroth-order estimate
    g z of a local step lands in ``.grad`` with no buffer beyond the generator windows --; more
    seeds run through a bounded f32 staging area (codec.expand_mt_multi).  Row m equals the
    single call bit for bit; torch's generators are left alone."""
    params = [p for g in param_groups for p in g["params"]]
    if not params or codec.resolve_stream_mode(params[0].device, stream_mode) != "torch_cpu":
        return seed_expansions_(param_groups, seeds, scalar_lists, output_lists, accumulate=accumulate,
                                stream_mode=stream_mode)
    if params[0].device.type != "cuda":  # before any output is created: there is no CPU path
        raise ValueError(f"FedKSeed codec: parameters must be on a HIP device (got {params[0].device}); "
                         "there is no CPU path")
    scalar_lists = [list(c) for c in scalar_lists]
    output_lists = list(output_lists)
    if len(scalar_lists) != len(output_lists):
        raise ValueError(f"one scalar list per output list: {len(output_lists)} output lists, "
                         f"{len(scalar_lists)} scalar lists")
    outs = [_expansion_outputs(params, o, m) for m, o in enumerate(output_lists)]
    if not outs:
        return outs
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    betas = [1.0 if accumulate else 0.0] * len(outs)
    detached = [[None if o is None else o.detach() for o in os_] for os_ in outs]
    codec.expand_mt_multi(specs, seeds, scalar_lists, detached, betas=betas)
    return outs


def seed_expansion_on_stream_(param_groups: List[dict], seeds: Sequence[int], scalars: Sequence[float], outputs=None,
                              accumulate: bool = False, stream_mode=None):
    """``seed_expansion_`` on either stream (``seed_expansions_on_stream_`` for one output):
    sum_k scalars[k] z_k written, or added with ``accumulate``, into ``outputs`` -- by default
    every parameter's ``.grad`` --, z_k the stream the call resolves to on the parameters' device.
    Returns the list of outputs."""
    return seed_expansions_on_stream_(param_groups, seeds, [list(scalars)], [outputs], accumulate=accumulate,
                                      stream_mode=stream_mode)[0]


def build_seed_candidates(k, low=0, high=2**32):
    """K seed candidates drawn from the global torch generator."""
    return torch.randint(low, high, size=(k,), dtype=torch.long)


def get_even_seed_probabilities(k):
    """Uniform sampling probabilities 1/k."""
    return torch.ones(k) / k
