'''Context schedules without a device: known answers of the per-step (k, w), the argument errors, the unchanged signatures of Runner.gen /
compose beside the new gen_scheduled / compose_styled, `style_linear=None` as today's CompositeGuide, and a numpy restatement of the
fd_lerp_f16 arithmetic contract with its exact cases.'''
import inspect

import numpy as np
import pytest
import torch

from flexdiffuse_amd.ctx_schedule import check_keyframes, locate, schedule_values, step_weights


def close(got, want):
    assert [k for k, _ in got] == [k for k, _ in want], (got, want)
    assert np.allclose([w for _, w in got], [w for _, w in want], rtol=0, atol=1e-15), (got, want)


# ---- (k, w) per step -------------------------------------------------------------------------------------------------
def test_two_keyframes_linear():
    close(step_weights(5), [(0, 0.0), (0, 0.25), (0, 0.5), (0, 0.75), (0, 1.0)])
    # progress_j = j / (steps - 1) exactly, in Python float
    assert step_weights(10) == [(0, j / 9) for j in range(10)]
    assert step_weights(10)[0] == (0, 0.0) and step_weights(10)[-1] == (0, 1.0)
    close(step_weights(3, schedule=(0.8, 0.2)), [(0, 0.8), (0, 0.5), (0, 0.2)])          # the reverse fade


def test_three_keyframes_even_and_uneven_positions():
    # even positions (0, 0.5, 1): s = 0, 0.25, 0.5, 0.75, 1 -- s == p_1 opens segment 1 at w = 0, s == 1 closes the last at w = 1
    close(step_weights(5, 3), [(0, 0.0), (0, 0.5), (1, 0.0), (1, 0.5), (1, 1.0)])
    # uneven (0, 0.25, 1)
    close(step_weights(5, 3, positions=(0.0, 0.25, 1.0)), [(0, 0.0), (1, 0.0), (1, 1 / 3), (1, 2 / 3), (1, 1.0)])
    close(step_weights(3, 4, positions=(0.0, 0.1, 0.9, 1.0)), [(0, 0.0), (1, 0.5), (2, 1.0)])
    assert locate(0.125, (0.0, 0.25, 1.0)) == (0, 0.5)


def test_one_step_and_img2img_offset():
    assert step_weights(1) == [(0, 0.0)]                       # progress is 0 when steps == 1
    assert step_weights(1, schedule=(0.3, 0.9)) == [(0, 0.3)]
    # img2img at strength 0.6 over 10 steps starts at global step 4: the request's first weight is s_4, not s_0
    w = step_weights(10)
    assert w[4] == (0, 4 / 9) and [w[j] for j in range(4, 10)] == [(0, j / 9) for j in range(4, 10)]


def test_explicit_list_and_extrapolation():
    s = [0.0, 1.0, 0.5, 0.5, 0.25]
    assert schedule_values(5, s) == s
    close(step_weights(5, schedule=s), [(0, 0.0), (0, 1.0), (0, 0.5), (0, 0.5), (0, 0.25)])
    # outside [0, 1]: the first / last segment, extrapolated (negative guidance, overshoot)
    close(step_weights(3, schedule=(-0.5, 1.5)), [(0, -0.5), (0, 0.5), (0, 1.5)])
    close(step_weights(3, 3, schedule=(-0.25, 1.25)), [(0, -0.5), (1, 0.0), (1, 1.5)])
    close(step_weights(2, 3, schedule=(-1.0, 2.0), positions=(0.0, 0.2, 1.0)), [(0, -5.0), (1, 2.25)])


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_value_errors():
    a, b = torch.zeros(2, 77, 8), torch.zeros(2, 77, 8)
    assert check_keyframes([a, b]) == (2, 77, 8)
    with pytest.raises(ValueError, match='shape'):
        check_keyframes([a, torch.zeros(2, 76, 8)])
    with pytest.raises(ValueError, match='at least 2'):
        check_keyframes([a])
    with pytest.raises(ValueError, match='at least 2'):
        step_weights(5, 1)
    with pytest.raises(ValueError, match='rise strictly'):
        step_weights(5, 3, positions=(0.0, 0.7, 0.6))
    with pytest.raises(ValueError, match='rise strictly'):
        step_weights(5, 3, positions=(0.0, 0.5, 0.9))
    with pytest.raises(ValueError, match='positions for'):
        step_weights(5, 3, positions=(0.0, 1.0))
    with pytest.raises(ValueError, match='one weight per step'):
        step_weights(5, schedule=[0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match='mode'):
        from flexdiffuse_amd.ctx_schedule import resolve_mode
        resolve_mode('gemm')


class _Enc():
    def prompt(self, p):
        g = torch.Generator().manual_seed(sum(map(ord, p)) + 7 * len(p))
        return torch.randn((1, 77, 16), generator=g)


def test_scheduled_guide_argument_errors_and_cfg_stack():
    from flexdiffuse_amd.ctx_schedule import blend_f32
    from flexdiffuse_amd.pipeline.guide import ScheduledGuide, SimpleGuide
    enc = _Enc()
    a, b = torch.cat([enc.prompt('a'), enc.prompt('b')]), torch.cat([enc.prompt('c'), enc.prompt('d')])
    with pytest.raises(ValueError):
        ScheduledGuide(enc, None, 8.0, 10, [a])
    with pytest.raises(ValueError):
        ScheduledGuide(enc, None, 8.0, 10, [a, b[:1]])
    with pytest.raises(ValueError):
        ScheduledGuide(enc, None, 8.0, 10, [a, b], schedule=[0.0] * 9)
    g = ScheduledGuide(enc, None, 8.0, 10, [a, b], mode='project')
    assert type(g).noise_pred is SimpleGuide.noise_pred and g.batch_size == 2 and g.weights == step_weights(10)
    un = enc.prompt('').expand(2, -1, -1)
    assert torch.equal(g.context.keyframes[0], torch.cat([un, a])) and torch.equal(g.context.keyframes[1], torch.cat([un, b]))
    # the project route on the host: one stable handle, rewritten in place with the step's fp32 blend
    h = g.stacked_embeds()
    assert torch.equal(h, g.context.keyframes[0])
    g.at_step(3)
    assert g.stacked_embeds() is h and g.context.trace == [(3, 0, 3 / 9)]
    assert torch.equal(h, blend_f32(g.context.keyframes[0], g.context.keyframes[1], 3 / 9))
    assert torch.equal(h[:2], un)                       # CFG rows: a == b gives a
    g1 = ScheduledGuide(enc, None, 1.0, 10, [a, b], mode='project')
    assert torch.equal(g1.context.keyframes[1], b)


# ---- public signatures -----------------------------------------------------------------------------------------------
GEN = [('prompt', ''), ('init_image', None), ('guide', None), ('init_size', (512, 512)), ('mapping_concepts', ''),
       ('guide_threshold_mult', 0.5), ('guide_threshold_floor', 0.5), ('guide_clustered', 0.5), ('guide_linear', (0.0, 0.5)),
       ('guide_max_guidance', 0.5), ('guide_header_max', 0.15), ('guide_mode', 0), ('guide_reuse', True), ('strength', 0.6),
       ('steps', 10), ('guidance_scale', 8), ('samples', 1), ('seed', None), ('debug', False)]
COMPOSE = [('bg_prompt', ''), ('entities_df', ()), ('start_style', ''), ('end_style', ''), ('style_blend', (0.0, 1.0)),
           ('init_image', None), ('batches', 4), ('strength', 0.7), ('steps', 30), ('guidance_scale', 8.0),
           ('init_size', (512, 512)), ('seed', None), ('debug', False)]


def test_runner_signatures_unchanged_and_scheduled_entry_points():
    '''`gen` and `compose` keep the signatures their own tests pin (`mask_image` last); the schedule arrives through
    `gen_scheduled` / `compose_styled`, whose own arguments are keyword-only and which bind everything else to the
    pinned signatures.'''
    from flexdiffuse_amd.utils import Runner
    P = inspect.Parameter
    for fn, positional, kw in ((Runner.gen, GEN, {'mask_image': None}),
                               (Runner.compose, COMPOSE, {'batch_size': 1, 'masks': None, 'mask_image': None})):
        ps = list(inspect.signature(fn).parameters.values())[1:]
        assert [(p.name, p.default) for p in ps if p.kind is P.POSITIONAL_OR_KEYWORD] == positional
        assert {p.name: p.default for p in ps if p.kind is P.KEYWORD_ONLY} == kw
        assert len(ps) == len(positional) + len(kw) and ps[-1].name == 'mask_image'
    ps = inspect.signature(Runner.gen_scheduled).parameters
    assert [(n, p.kind) for n, p in ps.items()][1:] == [('prompt', P.POSITIONAL_OR_KEYWORD), ('end_prompt', P.KEYWORD_ONLY),
                                                         ('end_guide', P.KEYWORD_ONLY), ('schedule', P.KEYWORD_ONLY),
                                                         ('gen_args', P.VAR_KEYWORD)]
    assert ps['end_prompt'].default is None and ps['schedule'].default == (0.0, 1.0)
    ps = inspect.signature(Runner.compose_styled).parameters
    assert [(n, p.default) for n, p in ps.items() if p.kind is P.POSITIONAL_OR_KEYWORD][1:] == COMPOSE[:5]
    assert ps['style_linear'].kind is P.KEYWORD_ONLY and ps['style_linear'].default == (0.0, 0.5)

    class Recorder(Runner):
        def __init__(self):
            self.calls = []

        def _gen(self, given, travel=None):
            self.calls.append((given, travel))

        def _compose(self, given, style_linear=None):
            self.calls.append((given, style_linear))
    r = Recorder()
    r.gen('a', steps=7)
    r.gen_scheduled('a', end_prompt='b', schedule=(0.2, 0.8), steps=7, mask_image='m')
    (g0, t0), (g1, t1) = r.calls
    assert t0 is None and t1[0] == 'b' and t1[2] == (0.2, 0.8)
    assert {k: v for k, v in g1.items() if k not in ('self', 'mask_image')} == {k: v for k, v in g0.items() if k not in ('self', 'mask_image')}
    assert g1['mask_image'] == 'm' and g0['steps'] == 7 and g0['strength'] == 0.6
    with pytest.raises(TypeError):
        r.gen_scheduled('a', stepz=3)
    r.calls = []
    r.compose('bg', [], 'oil', 'photo', (0.1, 0.9), batches=1)
    r.compose_styled('bg', [], 'oil', 'photo', (0.1, 0.9), batches=1, style_linear=(0.0, 0.3))
    (c0, s0), (c1, s1) = r.calls
    assert s0 is None and s1 == (0.0, 0.3)
    assert {k: v for k, v in c1.items() if k != 'self'} == {k: v for k, v in c0.items() if k != 'self'} and c0['steps'] == 30


def test_composite_guide_signature_and_style_linear_none():
    '''Without `style_linear` the style prompts are encoded nowhere and `embed_tensor` is today's rep-major stack.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    ps = list(inspect.signature(CompositeGuide.__init__).parameters.values())
    assert [p.name for p in ps][:7] == ['self', 'encoder', 'unet', 'guidance', 'schema', 'steps', 'batch_size']
    assert {p.name: p.default for p in ps}['style_linear'] is None

    class Counting(_Enc):
        def __init__(self):
            self.seen = []

        def prompt(self, p):
            self.seen.append(p)
            return _Enc.prompt(self, p)
    enc = Counting()
    schema = Schema('a forest', 'oil painting', 'photograph', (0.0, 1.0), [EntitySchema('a deer', (8, 16), (64, 48), 0.8)])
    for B in (1, 2):
        enc.seen = []
        g = CompositeGuide(enc, None, 8.0, schema, 10, batch_size=B)
        assert enc.seen == ['', 'a forest', 'a deer'] and g.context is None
        rows = [enc.prompt(''), enc.prompt('a forest'), enc.prompt('a deer')]
        want = torch.cat([r.float().expand(B, -1, -1) for r in rows]).contiguous()
        assert torch.equal(g.embed_tensor, want) and g.stacked_embeds() is g.embed_tensor
        g.at_step(0)                                          # nothing to do
    # opted in: two keyframes, the unconditional block untouched, every other block pulled towards the style per token
    g = CompositeGuide(enc, None, 8.0, schema, 10, batch_size=2, style_linear=(0.0, 0.5), mode='project')
    k0, k1 = g.context.keyframes
    assert torch.equal(k0[:2], g.embed_tensor[:2]) and torch.equal(k1[:2], g.embed_tensor[:2])
    om = torch.linspace(0.0, 0.5, 77).view(1, 77, 1)
    E = g.embed_tensor[2:]
    assert torch.equal(k0[2:], E + om * (enc.prompt('oil painting') - E)) and torch.equal(k1[2:], E + om * (enc.prompt('photograph') - E))
    assert torch.equal(k0[2:, 0], E[:, 0]) and g.context.weights == step_weights(10)


# ---- the arithmetic contract of fd_lerp_f16 --------------------------------------------------------------------------
def lerp_ref(a, b, w):
    '''half_rn(float(a) + w (float(b) - float(a))): three separately rounded fp32 operations; w == 0 / w == 1 are copies.'''
    w = np.float32(w)
    if w == 0:
        return a.copy()
    if w == 1:
        return b.copy()
    af, bf = a.astype(np.float32), b.astype(np.float32)
    return (af + w * (bf - af)).astype(np.float16)


def bits(x):
    return x.view(np.uint16)


def test_lerp_contract_exact_cases():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4096).astype(np.float16)
    a[:64] = (np.arange(1, 65) * 2.0 ** -24).astype(np.float16)            # subnormal halves
    a[64:68] = [65504.0, -65504.0, 0.0, 6.0e-8]
    b = rng.standard_normal(4096).astype(np.float16)
    b[:64] = (np.arange(64, 0, -1) * 2.0 ** -24).astype(np.float16) * np.float16(-1)
    b[2048:] = (a[2048:].astype(np.float32) * 3000).astype(np.float16)      # |b| = 3000 |a|
    big, small = b.copy(), a.copy()                                         # ... and the other way round: |a| >> |b|
    for x, y in ((a, b), (big, small)):
        assert np.array_equal(bits(lerp_ref(x, y, 0.0)), bits(x))
        assert np.array_equal(bits(lerp_ref(x, y, 1.0)), bits(y))
    for w in (0.37, -0.25, 1.5, 1e-3):
        assert np.array_equal(bits(lerp_ref(a, a, w)), bits(a)), w         # a == b gives a (no negative zero among the inputs)
        assert np.array_equal(bits(lerp_ref(big, big, w)), bits(big)), w
    # why w == 1 is a branch: the formula alone misses b where |a| >> |b|
    af, bf = big.astype(np.float32), small.astype(np.float32)
    formula = (af + np.float32(1.0) * (bf - af)).astype(np.float16)
    assert not np.array_equal(bits(formula), bits(small))
    # a zero of either sign blends to +0
    z = np.array([-0.0], np.float16)
    assert bits(lerp_ref(z, z, 0.5))[0] == 0 and bits(lerp_ref(z, z, 0.0))[0] == 0x8000
