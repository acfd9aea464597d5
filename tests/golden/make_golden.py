#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running the REFERENCE itself on CPU.

Runs only in the build container (needs /root/reference).  The reference's files never travel:
this script imports them, feeds them the seed-determined inputs of
``invertavatar_amd.synthetic`` and stores input/output vectors as .npz.  Three modules the
reference imports but the container lacks are stubbed: ``turtle``,
``torchvision`` (unused on the path) and ``cv2`` (only ``floodFill`` is reached; stubbed with
scipy.ndimage connected-component labelling, 4-connectivity).

Usage:  python tests/golden/make_golden.py [--only ops,camera,renderer,eg3d,small,extra,full,names,encoder,dataset]
"""
import argparse
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
REF = '/root/reference'
sys.path.insert(0, REPO)

from invertavatar_amd import synthetic  # noqa: E402


def install_stubs():
    import scipy.ndimage as ndi
    t = types.ModuleType('turtle')
    t.update = lambda *a, **k: None
    sys.modules['turtle'] = t
    tv = types.ModuleType('torchvision')
    tv.transforms = types.ModuleType('torchvision.transforms')
    sys.modules['torchvision'] = tv
    sys.modules['torchvision.transforms'] = tv.transforms
    cv2 = types.ModuleType('cv2')
    cv2.FLOODFILL_FIXED_RANGE = 1 << 16

    def flood_fill(img, mask, seed, new_val, lo, up, flags):
        x, y = seed
        sv = img[y, x]
        lab, _ = ndi.label((img >= sv - lo[0]) & (img <= sv + up[0]))
        img[lab == lab[y, x]] = new_val[0]
        return 0
    cv2.floodFill = flood_fill
    sys.modules['cv2'] = cv2


@contextlib.contextmanager
def injected_jitter(jit):
    """Replace torch.rand_like for the duration of one reference call (renderer.py:406)."""
    orig = torch.rand_like

    def fake(t, *a, **k):
        assert tuple(t.shape) == tuple(jit.shape), (t.shape, jit.shape)
        return jit.to(t.dtype)
    torch.rand_like = fake
    try:
        yield
    finally:
        torch.rand_like = orig


def npz(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
                                 for k, v in arrays.items()})
    print(f'{name}: {os.path.getsize(path) / 1e6:.2f} MB, {len(arrays)} arrays')


def rnd(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32))


# --------------------------------------------------------------------------------------------
def gen_ops():
    from torch_utils.ops import bias_act, upfirdn2d, conv2d_resample
    from training.networks_stylegan2 import modulated_conv2d
    import torch.nn.functional as F
    out = {}
    x = rnd(1, 2, 6, 9, 7) * 2
    b = rnd(2, 6)
    for act in bias_act.activation_funcs:
        out[f'bias_act/{act}'] = bias_act.bias_act(x, b, act=act)
    out['bias_act/lrelu_clamp'] = bias_act.bias_act(x, b, act='lrelu', gain=0.7, clamp=0.9)
    out['bias_act/linear_dim3'] = bias_act.bias_act(x, rnd(3, 7), dim=3, act='linear', gain=2.0)
    out['bias_act/nobias'] = bias_act.bias_act(x, None, act='lrelu', alpha=0.1)
    f = upfirdn2d.setup_filter([1, 3, 3, 1])
    out['filter/1331'] = f
    out['filter/sep8'] = upfirdn2d.setup_filter([1, 2, 3, 4, 4, 3, 2, 1], gain=2.0, flip_filter=True)
    xi = rnd(4, 2, 5, 13, 11)
    out['upfirdn2d/blur_pad1'] = upfirdn2d.upfirdn2d(xi, f, padding=[1, 1, 1, 1], gain=4)
    out['upfirdn2d/up2'] = upfirdn2d.upsample2d(xi, f)
    out['upfirdn2d/down2'] = upfirdn2d.downsample2d(xi, f)
    out['upfirdn2d/mixed'] = upfirdn2d.upfirdn2d(xi, rnd(5, 3, 5).abs(), up=[2, 3], down=[3, 2], padding=[2, -1, 0, 3],
                                                 flip_filter=True, gain=1.5)
    out['upfirdn2d/sep'] = upfirdn2d.upfirdn2d(xi, torch.tensor([1., 3., 3., 1.]) / 8, up=2, padding=[2, 1, 2, 1], gain=4)
    w = rnd(6, 8, 5, 3, 3)
    out['conv2d_resample/up2'] = conv2d_resample.conv2d_resample(xi, w, f, up=2, padding=1, flip_weight=False)
    out['conv2d_resample/plain'] = conv2d_resample.conv2d_resample(xi, w, f, up=1, padding=1, flip_weight=True)
    out['conv2d_resample/down2'] = conv2d_resample.conv2d_resample(xi, w, f, down=2, padding=1)
    styles = rnd(7, 2, 5) * 0.5 + 1
    noise = rnd(8, 26, 22) * 0.1
    out['modconv/up2_fused'] = modulated_conv2d(xi, w, styles, noise=noise, up=2, padding=1, resample_filter=f,
                                                flip_weight=False, fused_modconv=True)
    out['modconv/up2_unfused'] = modulated_conv2d(xi, w, styles, noise=noise, up=2, padding=1, resample_filter=f,
                                                  flip_weight=False, fused_modconv=False)
    out['modconv/plain_fused'] = modulated_conv2d(xi, w, styles, padding=1, fused_modconv=True)
    out['modconv/torgb'] = modulated_conv2d(xi, rnd(9, 3, 5, 1, 1), styles, demodulate=False, fused_modconv=True)
    img = rnd(10, 1, 4, 37, 41)
    out['resize_aa/down'] = F.interpolate(img, size=(16, 16), mode='bilinear', antialias=True)
    out['resize_aa/up'] = F.interpolate(img, size=(64, 50), mode='bilinear', antialias=True)
    grid = torch.from_numpy(np.random.RandomState(11).uniform(-1.2, 1.2, (1, 9, 10, 2)).astype(np.float32))
    out['grid_sample'] = F.grid_sample(img, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    npz('ops.npz', **out)


def gen_camera():
    import math
    from camera_utils import LookAtPoseSampler, FOV_to_intrinsics
    poses = [(math.pi / 2, math.pi / 2), (math.pi / 2 + 0.35, math.pi / 2 - 0.3), (1.1, 1.9)]
    mats = [LookAtPoseSampler.sample(y, p, torch.tensor([0, 0, 0.2]), radius=2.7)[0] for y, p in poses]
    npz('camera.npz', yaw_pitch=np.array(poses), cam2world=torch.stack(mats), intrinsics=FOV_to_intrinsics(18.837))


def gen_renderer():
    """Stage-level fixture: the reference's ImportanceRenderer_bsMotion + OSGDecoder + ray sampler on random planes."""
    from training_avatar_texture.triplane_v20 import OSGDecoder
    from training_avatar_texture.volumetric_rendering.renderer import ImportanceRenderer_bsMotion, fill_mouth
    from training_avatar_texture.volumetric_rendering.ray_sampler import RaySampler_zxc
    frames, nrr = [3, 77], 16
    planes = rnd(20, 2, 3, 32, 64, 64)
    dec = OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 32})
    synthetic.fill_parameters(dec, salt=5)
    cams = synthetic.camera_labels(frames)
    ro, rd = RaySampler_zxc()(cams[:, :16].view(-1, 4, 4), cams[:, 16:25].view(-1, 3, 3), nrr)
    jit = synthetic.jitter(frames, nrr * nrr)
    ren = ImportanceRenderer_bsMotion()
    rec = {'march': [], 'search': [], 'sort': [], 'fine': []}
    ren.ray_marcher.register_forward_hook(lambda m, i, o: rec['march'].append((i[0], i[1], i[2], o)))
    orig_search, orig_sort, orig_imp = torch.searchsorted, torch.sort, ren.sample_importance

    def search(cdf, u, **k):
        r = orig_search(cdf, u, **k)
        rec['search'].append((cdf, u, r))
        return r

    def sort(t, **k):
        r = orig_sort(t, **k)
        rec['sort'].append(r[1])
        return r

    def imp(*a, **k):
        r = orig_imp(*a, **k)
        rec['fine'].append(r)
        return r
    torch.searchsorted, torch.sort, ren.sample_importance = search, sort, imp
    try:
        with injected_jitter(jit):
            rgb, depth, wsum = ren(planes, dec, ro, rd, synthetic.rendering_kwargs(), evaluation=True)
    finally:
        torch.searchsorted, torch.sort = orig_search, orig_sort
    (cc, dc, zc, (_, _, wc)), (ca, da, za, _) = rec['march']
    cdf, u, inds = rec['search'][0]
    # known-answer set for fill_mouth: empty, full, ring with hole, hole touching the border, two holes
    masks = np.zeros((5, 1, 32, 32), np.float32)
    masks[1] = 1
    masks[2, 0, 6:26, 6:26] = 1; masks[2, 0, 12:18, 10:22] = 0
    masks[3, 0, 4:28, 4:28] = 1; masks[3, 0, 10:16, 0:14] = 0
    masks[4, 0, 3:29, 3:29] = 1; masks[4, 0, 8:12, 8:14] = 0; masks[4, 0, 18:24, 15:25] = 0
    full, mouth = fill_mouth(torch.from_numpy(masks).clone(), blur_mouth_edge=False)
    npz('renderer.npz', frames=np.array(frames), nrr=nrr, rays_o=ro, rays_d=rd, rgb=rgb, depth=depth, wsum=wsum,
        z_coarse=zc, den_coarse=dc, col_coarse=cc, w_coarse=wc, z_fine=rec['fine'][0], cdf=cdf, u=u, inds=inds,
        order=rec['sort'][0], z_all=za, den_all=da,
        fill_masks=masks, fill_full=full, fill_mouth=mouth)


EG3D_CASES = {   # name: (flip_z, ray_start, ray_end)   -- 'auto' = per-ray box limits (renderer.py:131-137)
    'auto': (False, 'auto', 'auto'),
    'auto_flip': (True, 'auto', 'auto'),
    'fixed': (False, 2.25, 3.3),
    'fixed_flip': (True, 2.25, 3.3),
}


def eg3d_inputs():
    """Inputs of the R9 fixture: two orbit cameras whose focal length is shortened (x 0.45) so that the corner rays MISS the
    tri-plane box (the `is_ray_valid` repair of renderer.py:133-136 is exercised), 12^2 rays, 48^2 planes."""
    frames, nrr = [3, 77], 12
    cams = synthetic.camera_labels(frames).clone()
    cams[:, 16] *= 0.45
    cams[:, 20] *= 0.45
    return frames, nrr, cams, rnd(21, 2, 3, 32, 48, 48)


def gen_renderer_eg3d():
    """R9: the reference's ImportanceRenderer (renderer.py:122-293) with flip_z in {False, True}, 'auto' and fixed ray limits.  Both
    random draws are pinned (fixed_randomness: stratified jitter :234/:238, uniform importance draws :453)."""
    from training_avatar_texture.triplane_v20 import OSGDecoder
    from training_avatar_texture.volumetric_rendering import math_utils
    from training_avatar_texture.volumetric_rendering.renderer import ImportanceRenderer
    from training_avatar_texture.volumetric_rendering.ray_sampler import RaySampler_zxc
    frames, nrr, cams, planes = eg3d_inputs()
    dec = OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 32})
    synthetic.fill_parameters(dec, salt=5)
    ro, rd = RaySampler_zxc()(cams[:, :16].view(-1, 4, 4), cams[:, 16:25].view(-1, 3, 3), nrr)
    jit = synthetic.jitter(frames, nrr * nrr)
    arrays = dict(frames=np.array(frames), nrr=nrr, cams=cams, rays_o=ro, rays_d=rd)
    t0, t1 = math_utils.get_ray_limits_box(ro, rd, box_side_length=1)
    arrays['box_near'], arrays['box_far'] = t0, t1
    assert (t1 > t0).any() and not (t1 > t0).all(), 'fixture needs both hitting and missing rays'
    for name, (flip, start, end) in EG3D_CASES.items():
        ren = ImportanceRenderer(flip_z=flip)
        rec = {'march': [], 'search': [], 'sort': []}
        ren.ray_marcher.register_forward_hook(lambda m, i, o: rec['march'].append((i[2], o[2])))
        orig_search, orig_sort = torch.searchsorted, torch.sort

        def search(cdf, u, **k):
            r = orig_search(cdf, u, **k)
            rec['search'].append((cdf, u, r))
            return r

        def sort(t, **k):
            r = orig_sort(t, **k)
            rec['sort'].append(r[1])
            return r
        torch.searchsorted, torch.sort = search, sort
        try:
            with fixed_randomness(jit):
                rgb, depth, wsum = ren(planes, dec, ro.clone(), rd.clone(), synthetic.rendering_kwargs(ray_start=start, ray_end=end))
        finally:
            torch.searchsorted, torch.sort = orig_search, orig_sort
        (zc, wc), _ = rec['march']
        cdf, u, inds = rec['search'][0]
        arrays.update({f'{name}/rgb': rgb, f'{name}/depth': depth, f'{name}/wsum': wsum, f'{name}/z_coarse': zc, f'{name}/w_coarse': wc,
                       f'{name}/u': u, f'{name}/inds': inds, f'{name}/order': rec['sort'][0]})
    npz('renderer_eg3d.npz', **arrays)


def g2_extra_inputs():
    """Inputs of the G2 fixture (synthesis_withCondition / sample / sample_mixed on the reduced-width generator)."""
    frames, nrr = [9, 130], 32
    cond = torch.stack([1 + 0.1 * rnd(31, 2, 16, 64, 64), 0.2 * rnd(32, 2, 16, 64, 64)])      # CS-SFT (scale, shift) at 64^2: C/2 = 16
    pts = torch.from_numpy(np.random.RandomState(33).uniform(-0.55, 0.55, (2, 700, 3)).astype(np.float32))
    dirs = torch.nn.functional.normalize(rnd(34, 2, 700, 3), dim=-1)
    return frames, nrr, cond, pts, dirs


def gen_generator_extra():
    """G2: the entry points of TriPlaneGenerator that no BASELINE config calls (triplane_v20.py:246-315, 341-402)."""
    g = build_reference_generator('small')
    frames, nrr, cond, pts, dirs = g2_extra_inputs()
    z = synthetic.latent(0, 2)
    c = synthetic.camera_labels(frames)
    uv = synthetic.uv_conditions(frames)
    ws = g.mapping(z, c, truncation_psi=0.7, truncation_cutoff=14)
    jit = synthetic.jitter(frames, nrr * nrr)
    arrays = dict(frames=np.array(frames), nrr=nrr, ws=ws)
    with injected_jitter(jit):
        out = g.synthesis_withCondition(ws, c, {'uvcoords_image': uv}, static_feats_conditions={64: cond}, neural_rendering_resolution=nrr,
                                        noise_mode='const', return_feats=True)
    arrays.update({'cond/image_sub4': sub4(out['image']), 'cond/image_raw': out['image_raw'], 'cond/image_depth': out['image_depth'],
                   'cond/feature_image': out['feature_image'], 'cond/triplane_s8': out['triplane'][..., ::8, ::8]})
    for kind in ('static', 'texture'):
        for i, t in enumerate(out[kind]):
            thin_into(arrays, f'cond/{kind}{i}', t, limit=20000)
    with injected_jitter(jit):
        only = g.synthesis_withCondition(ws, c, {'uvcoords_image': uv}, gt_texture_feats=None, neural_rendering_resolution=nrr,
                                         noise_mode='const', only_image=True)
    assert list(only.keys()) == ['image']
    arrays['cond_plain/image_sub4'] = sub4(only['image'])
    q = g.sample(pts.clone(), dirs, z, c, {'uvcoords_image': uv}, truncation_psi=0.7, truncation_cutoff=14, noise_mode='const')
    arrays['sample/rgb'], arrays['sample/sigma'] = q['rgb'], q['sigma']
    q = g.sample_mixed(pts.clone(), dirs, ws.flip(0).contiguous(), {'uvcoords_image': uv}, noise_mode='const')
    arrays['sample_mixed/rgb'], arrays['sample_mixed/sigma'] = q['rgb'], q['sigma']
    npz('generator_small_extra.npz', **arrays)


def build_reference_generator(width):
    from training_avatar_texture.triplane_v20 import TriPlaneGenerator
    g = TriPlaneGenerator(**synthetic.generator_kwargs(width)).eval().requires_grad_(False)
    synthetic.fill_parameters(g)
    return g


def sub4(t):
    return t[..., ::4, ::4]


def thin_into(arrays, name, t, limit=50000):
    """Spatial sub-sampling with the stride recorded in the key: <name>_s<stride>."""
    stride = 1
    while t[..., ::stride, ::stride].numel() > limit:
        stride *= 2
    arrays[f'{name}_s{stride}'] = t[..., ::stride, ::stride]


def gen_generator(width):
    g = build_reference_generator(width)
    frames = [5, 60] if width == 'small' else [5]
    nrr = 32 if width == 'small' else 64
    z = synthetic.latent(0, 1)
    ws = g.mapping(z, synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14).repeat(len(frames), 1, 1)
    c = synthetic.camera_labels(frames)
    uv = synthetic.uv_conditions(frames)
    jit = synthetic.jitter(frames, nrr * nrr)
    with injected_jitter(jit):
        out = g.synthesis(ws, c, {'uvcoords_image': uv}, neural_rendering_resolution=nrr, noise_mode='const',
                          evaluation=True, return_featmap=True)
    arrays = dict(frames=np.array(frames), nrr=nrr, ws=ws, image_raw=out['image_raw'], image_depth=out['image_depth'],
                  feature_image=out['feature_image'], triplane_sub4=sub4(out['triplane']))
    if width == 'small':
        arrays['image'] = out['image'][:1]
        arrays['image_sub4'] = sub4(out['image'])
        for i, t in enumerate(out['texture']):
            arrays[f'texture{i}'] = t if t.numel() < 300000 else sub4(t)
        # generator left in train() mode -> non-fused modulated conv (eval_seq.py:92)
        g.train()
        with injected_jitter(jit):
            out_t = g.synthesis(ws, c, {'uvcoords_image': uv}, neural_rendering_resolution=nrr, noise_mode='const', evaluation=True)
        g.eval()
        arrays['image_trainmode_sub4'] = sub4(out_t['image'])
        # drive-loop entry point with cached backbones (eval_seq.py:169-170,212)
        tex = g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, noise_mode='const')
        sta = g.backbone.synthesis(ws, cond_list=None, return_list=True, noise_mode='const')
        with injected_jitter(jit):
            out_w = g.synthesis_withTexture(ws, tex, c, {'uvcoords_image': uv}, static_feats=sta,
                                            neural_rendering_resolution=nrr, noise_mode='const', evaluation=True)
        arrays['image_withtexture_sub4'] = sub4(out_w['image'])
    else:
        arrays['image_sub4'] = sub4(out['image'])
        arrays['image_mean_abs'] = out['image'].abs().mean()
    npz(f'generator_{width}.npz', **arrays)


def block_means(t, k=32):
    """Mean of every k x k block: a position-sensitive checksum of a full-resolution image."""
    return torch.nn.functional.avg_pool2d(t.double(), k).float()


def gen_generator_bench():
    """The configuration bench.py times (BASELINE configs[1]): full width, nrr = 128, 512^2 out, B = 1 per call, plus one
    B = 2 call (batch-global `dist`, renderer.py:311: the coupling config 4's sharding must reproduce)."""
    g = build_reference_generator('full')
    nrr, frames = 128, [0, 17]
    ws1 = g.mapping(synthetic.latent(0, 1), synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14)
    arrays = dict(frames=np.array(frames), nrr=nrr, ws=ws1)

    def record(tag, out):
        img = out['image']
        arrays[f'{tag}_image_sub4'] = sub4(img)
        arrays[f'{tag}_image_crop'] = img[..., 224:288, 224:288]
        arrays[f'{tag}_image_block_means'] = block_means(img)
        arrays[f'{tag}_image_raw'] = out['image_raw']
        arrays[f'{tag}_image_depth_sub2'] = out['image_depth'][..., ::2, ::2]
    for k in frames:
        jit = synthetic.jitter([k], nrr * nrr)
        with injected_jitter(jit):
            out = g.synthesis(ws1, synthetic.camera_labels([k]), {'uvcoords_image': synthetic.uv_conditions([k])},
                              neural_rendering_resolution=nrr, noise_mode='const', evaluation=True)
        record(f'f{k}', out)
    jit = synthetic.jitter(frames, nrr * nrr)
    with injected_jitter(jit):
        out = g.synthesis(ws1.repeat(2, 1, 1), synthetic.camera_labels(frames), {'uvcoords_image': synthetic.uv_conditions(frames)},
                          neural_rendering_resolution=nrr, noise_mode='const', evaluation=True)
    record('b2', out)
    npz('generator_full_nrr128.npz', **arrays)


@contextlib.contextmanager
def fp16_blocks_on_cpu():
    """The reference forces every SynthesisBlock to fp32 when its tensors are not on a CUDA device (training/networks_stylegan2.py:421-422).
    For ONE fixture the check is taken out of SynthesisBlock.forward (the method's own source, compiled with that line replaced, in this
    process only), so that the blocks built with use_fp16 run the reference's fp16 path -- its own rounding points: x, w * s * d and every
    stored tensor in fp16, conv_clamp 256 -- on CPU tensors.  Backbones (g_num_fp16_res = 0) are unaffected."""
    import inspect
    import textwrap
    import training.networks_stylegan2 as ref_sg2
    base = ref_sg2.SynthesisBlock
    base = [c for c in base.__mro__ if 'forward' in c.__dict__][0]
    needle = "if ws.device.type != 'cuda':"
    src = textwrap.dedent(inspect.getsource(base.forward))
    assert src.count(needle) == 1, 'the device check of SynthesisBlock.forward moved'
    ns = dict(sys.modules[base.__module__].__dict__)
    exec(src.replace(needle, 'if False:'), ns)
    orig, base.forward = base.forward, ns['forward']
    try:
        yield
    finally:
        base.forward = orig


def gen_sr_fp16():
    """VERDICT r5 hygiene 9b: the SR head in its DEPLOYED precision (sr_num_fp16_res = 4, train_avatar_texture.py:215) pinned to the reference's
    own fp16 arithmetic.  Inputs: seeded features [1,32,128,128] (rnd(31) * 0.5) and the mapped ws; outputs of the reference head in fp16
    mode (device check lifted, see fp16_blocks_on_cpu) and in the fp32 mode it takes on CPU otherwise."""
    from training_avatar_texture.triplane_v20 import TriPlaneGenerator
    g = TriPlaneGenerator(**synthetic.generator_kwargs('full', sr_num_fp16_res=4)).eval().requires_grad_(False)
    synthetic.fill_parameters(g)
    feat = rnd(31, 1, 32, 128, 128) * 0.5
    ws = g.mapping(synthetic.latent(0, 1), synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14)
    nm = g.rendering_kwargs['superresolution_noise_mode']
    with fp16_blocks_on_cpu():
        img16 = g.superresolution(feat[:, :3].contiguous(), feat, ws, noise_mode=nm).float()
    img32 = g.superresolution(feat[:, :3].contiguous(), feat, ws, noise_mode=nm).float()
    assert (img16 - img32).abs().max().item() > 1e-4, 'the fp16 path did not run'
    arrays = dict(ws=ws)
    for tag, img in (('fp16', img16), ('fp32', img32)):
        arrays[f'{tag}_image_sub4'] = sub4(img)
        arrays[f'{tag}_image_crop'] = img[..., 224:288, 224:288]
        arrays[f'{tag}_image_block_means'] = block_means(img)
    npz('sr_fp16.npz', **arrays)


FLR_CASES = {   # name: (shape, fu taps (0 = None; negative = 2-D of that size), fd taps, up, down, padding, gain, slope, clamp, flip)
    'sg3_up2_down2': ((2, 3, 20, 24), 12, 12, 2, 2, [10, 11, 9, 10], 2 ** 0.5, 0.2, 256.0, False),
    'up4_down2_flip': ((1, 4, 9, 13), 8, 6, 4, 2, [5, 6, 7, 4], 1.7, 0.1, None, True),
    'up2_only_2d': ((1, 2, 16, 16), -4, 0, 2, 1, [2, 1, 2, 1], 2 ** 0.5, 0.2, 0.8, False),
    'down2_only': ((2, 2, 33, 31), 0, 5, 1, 2, 0, 1.0, 0.3, None, False),
    'identity_filters': ((1, 3, 7, 9), 0, 0, 1, 1, [1, -1, 0, 2], 2 ** 0.5, 0.2, 1.0, False),
    'crop_negative_pad': ((1, 2, 24, 24), 6, 6, 2, 2, [-3, 4, 2, -1], 2 ** 0.5, 0.2, None, False),
}


def gen_filtered_lrelu():
    """Outputs of the reference's own definition of the op (_filtered_lrelu_ref = what filtered_lrelu() evaluates on CPU)."""
    from torch_utils.ops import filtered_lrelu as flr
    arrays = {}
    for i, (name, (shape, nu, nd, up, down, pad, gain, slope, clamp, flip)) in enumerate(FLR_CASES.items()):
        x = rnd(300 + i, *shape)
        b = rnd(320 + i, shape[1]) * 0.5
        mk = lambda seed, n: None if n == 0 else (rnd(seed, -n, -n).abs() / n ** 2 if n < 0 else rnd(seed, n).abs() / n)   # noqa: E731
        fu, fd = mk(340 + i, nu), mk(360 + i, nd)
        y = flr.filtered_lrelu(x, fu=fu, fd=fd, b=b, up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp, flip_filter=flip,
                               impl='ref')
        arrays[f'{name}/x'], arrays[f'{name}/b'], arrays[f'{name}/y'] = x, b, y
        if fu is not None: arrays[f'{name}/fu'] = fu
        if fd is not None: arrays[f'{name}/fd'] = fd
    npz('filtered_lrelu.npz', **arrays)


def import_reference_script(name):
    """Import one of the reference's top-level scripts (reenact_avatar_next3d.py, eval_seq.py) for its helpers.  Modules the
    scripts import at the top but the container lacks (imageio, torchvision.utils, the FaceVerse / pytorch3d renderer, the
    dataset classes' cv2 use) are stubbed as empty modules: only pure-torch helpers are called."""
    import importlib
    for mod in ('imageio', 'torchvision.utils', 'data_preprocess', 'data_preprocess.FaceVerse', 'data_preprocess.FaceVerse.renderer'):
        if mod not in sys.modules:
            sys.modules[mod] = types.ModuleType(mod)
    sys.modules['torchvision'].utils = sys.modules['torchvision.utils']
    sys.modules['data_preprocess.FaceVerse.renderer'].Faceverse_manager = object
    return importlib.import_module(name)


def gen_harness():
    """H1 (reenact_avatar_next3d.py:146-219) on the reduced-width generator: seeds -> z -> mapping(psi 0.7, cutoff 14) with the
    script's conditioning camera -> per drive frame one synthesis per seed -> the script's own layout_grid (uint8 HWC mosaic
    [target | seed 0 | seed 1]).  Also layout_grid alone on a seeded batch in every mode."""
    R = import_reference_script('reenact_avatar_next3d')
    from training_avatar_texture.camera_utils import LookAtPoseSampler, FOV_to_intrinsics
    arrays = {}
    x = rnd(77, 6, 3, 8, 12) * 1.2
    arrays['grid_in'] = x
    arrays['grid_3x2_hwc'] = R.layout_grid(x, grid_w=3, grid_h=2)
    arrays['grid_6x1_chw'] = R.layout_grid(x, grid_w=None, grid_h=1, chw_to_hwc=False)
    arrays['grid_1x6_hwc'] = R.layout_grid(x, grid_w=1, grid_h=6)
    assert R.parse_range('1,2,5-7') == [1, 2, 5, 6, 7] and R.parse_tuple('4x2') == (4, 2) and R.parse_tuple('0,1') == (0, 1)
    g = build_reference_generator('small')
    seeds, frames, nrr, psi, cutoff = [0, 3], [5, 60], 32, 0.7, 14
    g.neural_rendering_resolution = nrr
    intr = FOV_to_intrinsics(18.837)
    pose = LookAtPoseSampler.sample(np.pi / 2, np.pi / 2, torch.tensor(g.rendering_kwargs['avg_camera_pivot']), radius=g.rendering_kwargs['avg_camera_radius'])
    cond = torch.cat([pose.reshape(-1, 16), intr.reshape(-1, 9)], 1)
    ws = [g.mapping(torch.from_numpy(np.random.RandomState(sd).randn(1, g.z_dim)), cond, truncation_psi=psi, truncation_cutoff=cutoff)
          for sd in seeds]
    arrays.update(seeds=np.array(seeds), frames=np.array(frames), nrr=nrr, psi=psi, cutoff=cutoff, cond=cond, ws=torch.cat(ws))
    mosaics = []
    for k in frames:
        imgs = [synthetic.source_frames(1000 + k, 1)[0]]
        for w in ws:
            with injected_jitter(synthetic.jitter([k], nrr * nrr)):
                imgs.append(g.synthesis(w, synthetic.camera_labels([k]), {'uvcoords_image': synthetic.uv_conditions([k])}, noise_mode='const',
                                        evaluation=True)['image'][0])
        mosaics.append(R.layout_grid(torch.stack(imgs), grid_w=3, grid_h=1))
    m = np.stack(mosaics)
    arrays['mosaic_sub4'] = m[:, ::4, ::4]
    arrays['mosaic_crop'] = m[:, 192:320, 512 + 192:512 + 320]
    arrays['mosaic_sum'] = m.astype(np.int64).sum(axis=(1, 2))
    npz('harness.npz', **arrays)


@contextlib.contextmanager
def fixed_randomness(jit, u_seed=99):
    """Pin both noise sources of the renderer: the stratified jitter (torch.rand_like, renderer.py:406) and the uniform
    importance samples drawn when evaluation=False (torch.rand, renderer.py:453)."""
    orig_like, orig_rand = torch.rand_like, torch.rand

    def fake_like(t, *a, **k):
        assert tuple(t.shape) == tuple(jit.shape), (t.shape, jit.shape)
        return jit.to(t.dtype)

    def fake_rand(*size, **k):
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        t = torch.from_numpy(np.random.RandomState(u_seed).rand(*shape).astype(np.float32))
        return t.to(k['device']) if k.get('device') is not None else t
    torch.rand_like, torch.rand = fake_like, fake_rand
    try:
        yield
    finally:
        torch.rand_like, torch.rand = orig_like, orig_rand


def encoder_inputs(nrr=32):
    groups = [[0, 8, 16, 24], [4, 12, 20, 28]]
    data = []
    for gi, frames in enumerate(groups):
        data.append(dict(image=synthetic.source_frames(7 + gi, 4), uv=synthetic.source_uv(17 + gi, frames),
                         c=synthetic.camera_labels(frames), uvcoords=synthetic.uv_conditions(frames),
                         jitter=synthetic.jitter(frames, nrr * nrr)))
    drive = [40]
    return data, dict(c=synthetic.camera_labels(drive), uvcoords=synthetic.uv_conditions(drive), jitter=synthetic.jitter(drive, nrr * nrr))


def set_eval_seq_modes(net):
    """Module modes exactly as eval_seq.py:92-97 leaves them."""
    net.train()
    for unet in (net.unet_encoder.triplane_unet, net.unet_encoder.texture_unet):
        unet.input_layer.eval()
        unet.body.eval()
    return net


def run_few_shot(net, nrr=32, nrr_drive2=128):
    """eval_seq.py:168-212 as the script runs it on 8 sources (default arguments): encode the first source, features of
    that identity, then num_iter = 2 groups of four taken INTERLEAVED (``[idx::num_iter]``, :183-186), every group started from the
    e4e features (``e4e_results=e4e_results``, :187) with the ConvGRU states carried; the drive loop uses the LAST group's result.
    Two drive frames: one at the inversion's neural rendering resolution and one at `nrr_drive2` (the deployed 128)."""
    net.generator.neural_rendering_resolution = nrr
    groups, drive = encoder_inputs(nrr)
    src = {k: torch.cat([grp[k] for grp in groups]) for k in groups[0]}
    g = net.generator
    ws = net.encode(src['image'][:1])
    tex = g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')
    sta = g.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')
    e4e, r_list = {'w': ws, 'texture': tex, 'static': sta}, [None, None]
    num_iter = src['image'].shape[0] // 4
    for idx in range(num_iter):
        sel = slice(idx, None, num_iter)
        with fixed_randomness(src['jitter'][sel]):
            res, r_list = net.AR_eval_forward({'image': src['image'][sel], 'uv': src['uv'][sel]}, src['c'][sel],
                                              {'uvcoords_image': src['uvcoords'][sel]}, ws, r_list, e4e_results=e4e, return_fake=False)
    with fixed_randomness(drive['jitter']):
        out = g.synthesis_withTexture(ws, res['texture'], drive['c'], {'uvcoords_image': drive['uvcoords']}, noise_mode='const',
                                      static_feats=res['static'], evaluation=True)
    d2 = drive_frame2(nrr_drive2)
    with fixed_randomness(d2['jitter']):
        out2 = g.synthesis_withTexture(ws, res['texture'], d2['c'], {'uvcoords_image': d2['uvcoords']}, noise_mode='const',
                                       static_feats=res['static'], evaluation=True, neural_rendering_resolution=nrr_drive2)
    g.neural_rendering_resolution = nrr
    return ws, res, r_list, out['image'], out2['image']


def drive_frame2(nrr=128):
    fr = [47]
    return dict(c=synthetic.camera_labels(fr), uvcoords=synthetic.uv_conditions(fr), jitter=synthetic.jitter(fr, nrr * nrr))


def gen_encoder():
    from encoder_inversion.models.uvnet import inversionNet
    g = build_reference_generator('full')     # the UNet heads are sized for the full-width feature pyramid
    net = inversionNet(generator=g, encoding_triplane=True, encoding_texture=True).requires_grad_(False)
    synthetic.fill_encoder_parameters(net)
    set_eval_seq_modes(net)
    ws, res, r_list, image, image2 = run_few_shot(net)
    def thin(name, t):      # spatial sub-sampling with the stride recorded in the key: <name>_s<stride>
        stride = 1
        while t[..., ::stride, ::stride].numel() > 50000:
            stride *= 2
        arrays[f'{name}_s{stride}'] = t[..., ::stride, ::stride]
    arrays = dict(ws=ws)
    thin('drive_image', image)
    thin('drive_image_nrr128', image2)
    arrays['drive_image_nrr128_crop'] = image2[:, :, 192:320, 192:320]
    arrays['drive_image_nrr128_blockmean'] = block_means(image2)
    for i, t in enumerate(res['texture']):
        thin(f'texture{i}', t)
    for i, t in enumerate(res['static']):
        thin(f'static{i}', t)
    for u, states in enumerate(r_list):
        for k, h in enumerate(states):
            thin(f'gru{u}_{k}', h)
    npz('encoder_fewshot.npz', **arrays)
    lines = [f'{n}\t{tuple(t.shape)}\t{str(t.dtype).replace("torch.", "")}' for n, t in sorted(net.state_dict().items())
             if not n.startswith('generator.')]
    with open(os.path.join(HERE, 'encoder_state_names.txt'), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print(f'encoder_state_names.txt: {len(lines)} tensors')


def install_timm_stub():
    """mix_transformer.py imports three helpers from timm (absent here): identity DropPath at rate 0, to_2tuple, trunc_normal_."""
    class DropPath(torch.nn.Module):
        def __init__(self, drop_prob=0.):
            super().__init__()
            self.drop_prob = drop_prob

        def forward(self, x):
            assert self.drop_prob == 0. or not self.training
            return x
    layers = types.ModuleType('timm.models.layers')
    layers.DropPath, layers.to_2tuple, layers.trunc_normal_ = DropPath, (lambda v: v if isinstance(v, tuple) else (v, v)), torch.nn.init.trunc_normal_
    reg = types.ModuleType('timm.models.registry'); reg.register_model = lambda f: f
    vit = types.ModuleType('timm.models.vision_transformer'); vit._cfg = lambda **k: {}
    for name, mod in (('timm', types.ModuleType('timm')), ('timm.models', types.ModuleType('timm.models')), ('timm.models.layers', layers),
                      ('timm.models.registry', reg), ('timm.models.vision_transformer', vit)):
        sys.modules.setdefault(name, mod)


def one_shot_inputs(nrr=32):
    src, drive = [12], [40]
    return dict(image=synthetic.source_frames(9, 1), uv=synthetic.source_uv(19, src), c=synthetic.camera_labels(src),
                uvcoords=synthetic.uv_conditions(src), jitter=synthetic.jitter(src, nrr * nrr),
                drive_c=synthetic.camera_labels(drive), drive_uvcoords=synthetic.uv_conditions(drive), drive_jitter=synthetic.jitter(drive, nrr * nrr))


def gen_encoder_new():
    """eval_updated_os.py flow (:94-95,171-179,198) with the reference's uvnet_new.inversionNet: eval() mode, one source frame,
    one-shot forward, one drive frame."""
    install_timm_stub()
    from encoder_inversion.models.uvnet_new import inversionNet
    g = build_reference_generator('full')
    net = inversionNet(generator=g, encoding_triplane=True, encoding_texture=True).eval().requires_grad_(False)
    synthetic.fill_encoder_parameters(net)
    nrr = 32
    g.neural_rendering_resolution = nrr
    inp = one_shot_inputs(nrr)
    ws = net.encode(inp['image'])
    tex = g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')
    sta = g.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')
    with fixed_randomness(inp['jitter']):
        out = net({'image': inp['image'], 'uv': inp['uv']}, inp['c'], {'uvcoords_image': inp['uvcoords']},
                  e4e_results={'w': ws, 'texture': tex, 'static': sta}, return_feats=True)
    static = sta[:-1] + out['static'][-1:]
    with fixed_randomness(inp['drive_jitter']):
        img = g.synthesis_withTexture(ws, out['texture'], inp['drive_c'], {'uvcoords_image': inp['drive_uvcoords']}, noise_mode='const',
                                      static_feats=static, evaluation=True)['image']
    arrays = dict(ws=ws)

    def thin(name, t):
        stride = 1
        while t[..., ::stride, ::stride].numel() > 50000:
            stride *= 2
        arrays[f'{name}_s{stride}'] = t[..., ::stride, ::stride]
    thin('drive_image', img)
    for i, t in enumerate(out['texture']):
        thin(f'texture{i}', t)
    thin('static5', static[-1])
    npz('encoder_oneshot.npz', **arrays)
    lines = [f'{n}\t{tuple(t.shape)}\t{str(t.dtype).replace("torch.", "")}' for n, t in sorted(net.state_dict().items())
             if n.startswith('unet_encoder.')]
    with open(os.path.join(HERE, 'encoder_new_state_names.txt'), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print(f'encoder_new_state_names.txt: {len(lines)} tensors')


def gen_dataset():
    """Every item the reference's ImageFolderDataset returns for the directory tests/test_dataset_cpu.py writes (RGBA frames), in the
    three reader configurations of test_equal_to_the_reference_reader, flattened by that test's _flatten."""
    import importlib
    import pathlib
    import tempfile
    import PIL.Image
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import test_dataset_cpu as T
    sys.modules['cv2'].imread = lambda p, flag=1: np.asarray(PIL.Image.open(p).convert('L'))   # imread(path, 0) of a 1-channel PNG
    ref_mod = importlib.import_module('training_avatar_texture.dataset_new')
    out, cwd = {}, os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        path, names, _, _ = T._write_dataset(pathlib.Path(d), rgba=True)
        os.chdir(d)              # the UV face mask is read relative to the working directory
        try:
            for c, extra in enumerate(T.READER_CONFIGS):
                ref = ref_mod.ImageFolderDataset(**T._kwargs(path, **extra))
                out[f'{c}/len'] = np.int64(len(ref))
                out[f'{c}/label_shape'], out[f'{c}/image_shape'] = np.array(str(list(ref.label_shape))), np.array(str(list(ref.image_shape)))   # (may hold None)
                for i in range(len(ref)):
                    T._flatten(out, f'{c}/item{i}', ref[i])
                    T._flatten(out, f'{c}/by_name{i}', ref.get_by_name(names[i]))
        finally:
            os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, 'dataset_reference.npz'), **out)
    print(f'dataset_reference.npz: {len(out)} arrays')


def gen_names():
    """(name, shape, dtype) of every parameter/buffer: the checkpoint-compatibility contract."""
    for width, fname in (('full', 'generator_state_names.txt'), ('small', 'generator_state_names_small.txt')):
        g = build_reference_generator(width)
        lines = [f'{n}\t{tuple(t.shape)}\t{str(t.dtype).replace("torch.", "")}' for n, t in sorted(g.state_dict().items())]
        with open(os.path.join(HERE, fname), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
        print(f'{fname}: {len(lines)} tensors, {sum(p.numel() for p in g.parameters())} parameters')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='ops,flr,camera,renderer,eg3d,small,extra,full,bench,sr16,harness,names,encoder,encoder_new,dataset')
    args = ap.parse_args()
    install_stubs()
    sys.path.insert(0, REF)
    torch.manual_seed(0)
    todo = args.only.split(',')
    with torch.no_grad():
        if 'ops' in todo: gen_ops()
        if 'flr' in todo: gen_filtered_lrelu()
        if 'camera' in todo: gen_camera()
        if 'renderer' in todo: gen_renderer()
        if 'eg3d' in todo: gen_renderer_eg3d()
        if 'small' in todo: gen_generator('small')
        if 'extra' in todo: gen_generator_extra()
        if 'full' in todo: gen_generator('full')
        if 'bench' in todo: gen_generator_bench()
        if 'sr16' in todo: gen_sr_fp16()
        if 'harness' in todo: gen_harness()
        if 'names' in todo: gen_names()
        if 'encoder' in todo: gen_encoder()
        if 'encoder_new' in todo: gen_encoder_new()
        if 'dataset' in todo: gen_dataset()


if __name__ == '__main__':
    main()
