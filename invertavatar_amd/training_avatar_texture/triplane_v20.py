"""Next3D++ (v20) animatable tri-plane generator on the MI355X backend.

API mirror of the reference's training_avatar_texture/triplane_v20.py: ``TriPlaneGenerator`` with
``mapping`` (:64), ``synthesis`` (:89), ``synthesis_withTexture`` (:152), ``synthesis_withCondition`` (:246),
``rasterize`` (:317), ``sample`` / ``sample_mixed`` (:341,:373), ``forward`` (:404) and ``OSGDecoder`` (:415),
with the reference's parameter names, argument meaning and return-dict keys.

Pipeline of one frame:
  texture backbone + static backbone (StyleGAN2, fused MFMA convolutions)
  -> rasterize: UV lookup of the neural texture, AA resize, alpha blend over the static features, mouth fill
     on the GPU (``ia_fill_mouth``; the reference round-trips through cv2 on the host)
  -> face backbone conditioned on those maps -> 128^2 stitch pasted into plane 0 -> blended tri-planes
  -> fused importance renderer (``ia_render_rays``: one launch) -> 32-channel 128^2 feature image
  -> super-resolution head -> 512^2 RGB.

Differences from the reference that do not change results: the three copies of the "rasterize / face
backbone / blend / render / SR" tail (:116-150, :179-244, :277-315) are one method here; ``rasterize`` can
skip the two levels the face backbone never reads (networks_stylegan2_new.py:536-540 with end_layer 6);
the stratified-sampling noise can be injected (``jitter=``) for reproducible evaluation.
"""
import torch
import torch.nn.functional as F

from .. import _runtime, dnnlib, hipops
from ..torch_utils import persistence
from ..training.networks_stylegan2 import FullyConnectedLayer
from .networks_stylegan2_new import Generator as StyleGAN2Backbone_cond
from .volumetric_rendering.renderer import ImportanceRenderer, ImportanceRenderer_bsMotion, fill_mouth  # noqa: F401
from .volumetric_rendering.ray_sampler import RaySampler, RaySampler_zxc  # noqa: F401

BBOX_256 = [57, 185, 64, 192]   # face region of the frontal plane, in 256^2 pixels (triplane_v20.py:114)
N_COND_LEVELS_USED = 4          # cond_list entries the face backbone consumes
CL_COPIES_ON_TEXTURE_STREAM = True   # False: the rasteriser's stream makes them (ia_rasterize_level's own copy)
LAUNCH_ORDER = 'tmfs'           # capture order of the frame's four independent branches: m mouth fill + rays, f face-backbone head,
                                # t texture backbone, s static backbone (profiles/r04_ab_launch_order_sweep.txt: two clusters 9 % apart)

FRAME_STYLE_BATCH = True        # synthesis(): the styles of all three backbones + the SR head in one launch pair at the top of the frame

RENDER_WRITES_SR_INPUT = True   # the fused renderer also writes its features in the SR head's operand format (no ia_act_split between them)
SINGLE_STREAM = False           # True: no side streams (every launch of a frame in program order on the caller's stream); used by
                                # bench.py to time kernels without neighbours from other streams


class _FrameState:
    """Per-generator orchestration state of the device path (side streams, tensors handed between the stages of ONE frame).
    It lives outside the module (invertavatar_amd._runtime) so that copy.deepcopy / pickle / torch.save of a generator that has
    already rendered see parameters and buffers only."""

    def __init__(self):
        self.streams = {}
        self.side_rays = None
        self.tex_cl = None

    def stream(self, name, device):
        st = self.streams.get(name)
        if st is None or st.device != device:
            st = self.streams[name] = torch.cuda.Stream(device=device)
        return st


def _state(gen):
    holder = _runtime.state(gen)
    if not hasattr(holder, 'frame'):
        holder.frame = _FrameState()
    return holder.frame


class _LazyLevels:
    """cond_list whose entry k is produced (rasterised) the first time the face backbone reads it."""

    def __init__(self, n, make):
        self._n, self._make, self._have = n, make, {}

    def __len__(self):
        return self._n

    def __getitem__(self, k):
        if k not in self._have:
            self._have[k] = self._make(k)
        return self._have[k]



def _aa_resize(x, size):
    return F.interpolate(x, size=(size, size), mode='bilinear', antialias=True)


@persistence.persistent_class
class TriPlaneGenerator(torch.nn.Module):
    def __init__(self, z_dim, c_dim, w_dim, img_resolution, img_channels, topology_path=None, sr_num_fp16_res=0,
                 mapping_kwargs={}, rendering_kwargs={}, sr_kwargs={}, **synthesis_kwargs):
        super().__init__()
        self.z_dim = z_dim
        self.c_dim = c_dim
        self.w_dim = w_dim
        self.img_resolution = img_resolution
        self.img_channels = img_channels
        self.renderer = ImportanceRenderer_bsMotion()
        self.ray_sampler = RaySampler_zxc()
        common = dict(img_resolution=256, mapping_kwargs=mapping_kwargs, **synthesis_kwargs)
        self.texture_backbone = StyleGAN2Backbone_cond(z_dim, c_dim, w_dim, img_channels=32, **common)
        self.face_backbone = StyleGAN2Backbone_cond(z_dim, c_dim, w_dim, img_channels=32, **common)
        self.backbone = StyleGAN2Backbone_cond(z_dim, c_dim, w_dim, img_channels=32 * 3, mapping_ws=self.texture_backbone.num_ws,
                                               **common)
        self.superresolution = dnnlib.util.construct_class_by_name(
            class_name=rendering_kwargs['superresolution_module'], channels=32, img_resolution=img_resolution,
            sr_num_fp16_res=sr_num_fp16_res, sr_antialias=rendering_kwargs['sr_antialias'], **sr_kwargs)
        self.decoder = OSGDecoder(32, {'decoder_lr_mul': rendering_kwargs.get('decoder_lr_mul', 1), 'decoder_output_dim': 32})
        self.neural_rendering_resolution = 128
        self.rendering_kwargs = rendering_kwargs
        self.fill_mouth = True

    # ------------------------------------------------------------------ latent mapping
    def mapping(self, z, c, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        if self.rendering_kwargs['c_gen_conditioning_zero']:
            c = torch.zeros_like(c)
        c = c[:, :self.c_dim]   # drop expression labels
        return self.backbone.mapping(z, c * self.rendering_kwargs.get('c_scale', 0), truncation_psi=truncation_psi,
                                     truncation_cutoff=truncation_cutoff, update_emas=update_emas)

    # ------------------------------------------------------------------ helpers
    def _rays(self, c, neural_rendering_resolution):
        cam = c[:, -25:]
        if neural_rendering_resolution is None:
            neural_rendering_resolution = self.neural_rendering_resolution
        else:
            self.neural_rendering_resolution = neural_rendering_resolution
        origins, dirs = self.ray_sampler(cam[:, :16].view(-1, 4, 4), cam[:, 16:25].view(-1, 3, 3), neural_rendering_resolution)
        return origins, dirs, neural_rendering_resolution

    def _two_backbones(self, ws, update_emas, synthesis_kwargs, partial=False, order='ts', side_work=None):
        """The texture and the static backbone are independent: on the device they run on two streams of their own so that their
        latency-bound low-resolution layers (a handful of workgroups each at batch 1) overlap.

        partial=True (synthesis): the rasteriser consumes the taps level by level (32^2, 64^2, 128^2) and the face backbone
        consumes the rasterised levels block by block, so nothing waits for whole networks: both backbones record an event
        after every tap (`pending[2]`, `pending[3]`: tap count -> event) and _planes rasterises level k when the face
        backbone asks for it.  The 256^2 blocks are not consumed by the rasteriser at all; the caller joins the streams
        (`pending[0]` texture, `pending[1]` static) where the last taps are consumed (_planes: static, before the plane
        blend; synthesis: texture, at the end of the frame)."""
        def tex(**kw):
            return self.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **kw, **synthesis_kwargs)

        def sta(**kw):
            return self.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **kw, **synthesis_kwargs)
        if not (ws.is_cuda and not torch.is_grad_enabled()) or SINGLE_STREAM:
            for work in (side_work or {}).values():
                work()
            return tex(), sta(), None
        st = _state(self)
        main, t_stream, s_stream = torch.cuda.current_stream(ws.device), st.stream('texture', ws.device), st.stream('static', ws.device)
        tex_cl = [None] * N_COND_LEVELS_USED
        counts = tuple(range(2, N_COND_LEVELS_USED + 1))       # taps 0 and 1 (image and features at 32^2) appear together
        ev_tex, ev_sta = {n: torch.cuda.Event() for n in counts}, {n: torch.cuda.Event() for n in counts}

        def make_cl(feats):   # the rasteriser gathers from channels-last copies; make them on the texture stream
            for k, t in enumerate(feats[:N_COND_LEVELS_USED]):
                if tex_cl[k] is None and t.dtype == torch.float32:
                    tex_cl[k] = hipops.channels_last_copy(t)

        def tap_tex(feats):
            if CL_COPIES_ON_TEXTURE_STREAM:
                make_cl(feats)
            ev_tex[len(feats)].record(t_stream)
        if not partial:
            t_stream.wait_stream(main)
            with torch.cuda.stream(t_stream):
                texture_feats = tex()
                make_cl(texture_feats)
            static_feats = sta()
            main.wait_stream(t_stream)
            pending = None
        else:
            # a graph replay queues its nodes branch by branch in capture order, a few microseconds each, so the order the
            # branches are captured in decides when each starts: `order` names it (t texture, s static, others: side_work)
            made = {}
            for ch in order:
                if ch == 't':
                    t_stream.wait_stream(main)
                    with torch.cuda.stream(t_stream):
                        made['t'] = tex(_tap=(counts, tap_tex))
                elif ch == 's':
                    s_stream.wait_stream(main)
                    with torch.cuda.stream(s_stream):
                        made['s'] = sta(_tap=(counts, lambda feats: ev_sta[len(feats)].record(s_stream)))
                else:
                    side_work[ch]()
            texture_feats, static_feats = made['t'], made['s']
            pending = (t_stream, s_stream, ev_tex, ev_sta)
        for t in list(texture_feats) + [t for t in tex_cl if t is not None] + (list(static_feats) if partial else []):
            t.record_stream(main)
        st.tex_cl = (texture_feats, tex_cl)
        return texture_feats, static_feats, pending

    def _frame_styles(self, ws):
        """Every affine style vector and demodulation coefficient of the frame -- three backbones and the SR head, ~190 layers -- in
        ONE `ia_styles_demod` launch pair on the caller's stream before the branches fork (they were 2 launches at the head of each
        network's chain: 8 per frame, ~25 us in front of each backbone's first convolution).  Marks the networks so that their own
        batchers skip this `ws`; returns True when the SR head's styles were part of the batch."""
        if not (FRAME_STYLE_BATCH and ws.is_cuda and not torch.is_grad_enabled()):
            return False
        from ..training.networks_stylegan2 import _StyleBatcher
        st = _state(self)
        nets = [self.texture_backbone.synthesis, self.backbone.synthesis, self.face_backbone.synthesis]
        if any(n.num_ws > ws.shape[1] for n in nets):
            return False
        if getattr(st, 'style_batcher', None) is None:
            st.style_batcher = _StyleBatcher()
        blocks, offs, fixed = [], [], []
        for n in nets:
            b, o = n._style_blocks()
            blocks += b; offs += o; fixed += [None] * len(b)
        sr = self.superresolution.style_blocks() if hasattr(self.superresolution, 'style_blocks') else None
        if sr is not None:
            blocks += sr; offs += [0] * len(sr); fixed += [ws.shape[1] - 1] * len(sr)
        if not st.style_batcher.prepare(blocks, offs, ws.to(torch.float32), fixed_w=fixed):
            return False
        for n in nets:
            _runtime.state(n).styles_for = ws
        return sr is not None

    def _start_face_head(self, ws, update_emas, synthesis_kwargs, sr_styles_ready=False):
        """The 4^2..32^2 blocks of the face backbone depend only on ws; run them on a third stream under the other backbones."""
        if not (ws.is_cuda and not torch.is_grad_enabled()) or SINGLE_STREAM:
            return None
        main, side = torch.cuda.current_stream(ws.device), _state(self).stream('face_head', ws.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            x, img, first = self.face_backbone.synthesis.forward_head(ws, update_emas=update_emas, **synthesis_kwargs)
            if hasattr(self.superresolution, 'hoist_styles'):      # three small launches off the render -> SR chain
                self.superresolution.hoist_styles(ws, prepared=sr_styles_ready)
            done = torch.cuda.Event()
            done.record(side)
        x.record_stream(main)
        img.record_stream(main)
        return x, img, first, done

    def _start_mouth_fill(self, mesh_condition, rays=None):
        """The mouth-hole fill depends only on the UV mask, and its flood is a one-workgroup, latency-bound kernel:
        start it on a side stream at the top of the frame so that it runs underneath the backbone convolutions.
        `rays` = (c, neural_rendering_resolution, ray_dist): the camera rays and the batch mean of |ray origin| depend
        only on the cameras, so they are produced on the same side stream (_FrameState.side_rays)."""
        uv = mesh_condition['uvcoords_image']
        st = _state(self)
        st.side_rays = None
        if not (uv.is_cuda and not torch.is_grad_enabled()) or SINGLE_STREAM:
            return None
        main, side = torch.cuda.current_stream(uv.device), st.stream('mouth', uv.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            uv_c = uv.float().contiguous()
            alpha = uv_c[..., 2:].permute(0, 3, 1, 2).contiguous()
            full_alpha, mouth = fill_mouth(alpha, blur_mouth_edge=False)
            upper_c = self._upper_alpha(alpha, mouth).reshape(-1, uv.shape[1], uv.shape[2]).contiguous()
            extra = ()
            if rays is not None:
                c, nrr, ray_dist = rays
                origins, dirs, nrr = self._rays(c, nrr)
                if ray_dist is None:
                    ray_dist = torch.norm(origins, dim=-1).mean().reshape(1)     # (renderer.py:311), no host sync
                st.side_rays = (origins, dirs, nrr, ray_dist)
                extra = (origins, dirs, ray_dist)
            done = torch.cuda.Event()
            done.record(side)
        for t in (uv_c, alpha, full_alpha, mouth, upper_c) + tuple(t for t in extra if torch.is_tensor(t)):
            t.record_stream(main)
        return alpha, full_alpha, mouth, done, uv_c, upper_c

    @staticmethod
    def _upper_alpha(alpha, mouth):
        """Face alpha with the upper part of the mouth hole closed (reference :324-326)."""
        upper = mouth.clone()
        upper[:, :, :87] = 0
        return torch.clamp(alpha + upper, min=0, max=1)

    @staticmethod
    def _split_static(static_feats):
        """The static backbone emits 96 = 3 x 32 channels; levels 0 and 5 carry all three planes and the
        rasteriser only blends over plane 0 of them (:109-112, :180-181)."""
        b = static_feats[0].shape[0]
        plane = static_feats[-1].view(b, 3, 32, *static_feats[-1].shape[-2:])
        first = static_feats[0].view(b, 3, 32, *static_feats[0].shape[-2:])[:, 0]
        return [first] + list(static_feats[1:-1]) + [plane[:, 0]], plane

    def _blend_planes(self, stitch, full_alpha, static_plane):
        """Paste the 128^2-resized face stitch + alpha into the bbox of plane 0; planes 1-2 stay static (:119-128)."""
        if (stitch.is_cuda and stitch.dtype == torch.float32 and stitch.shape[1:] == (32, 256, 256) and not torch.is_grad_enabled()
                and static_plane.shape[1:] == (3, 32, 256, 256)):
            # fused AA-resize + paste + blend, emitted channels-last; returned as the NCHW-shaped view of that buffer
            b = stitch.shape[0]
            sta = static_plane.reshape(b, 96, 256, 256)
            sta = sta if sta.is_contiguous() else sta.contiguous()
            cl = hipops.blend_planes(stitch.contiguous(), full_alpha.reshape(b, 256, 256).contiguous(), sta, BBOX_256)
            return cl.permute(0, 1, 4, 2, 3)
        y0, y1, x0, x1 = BBOX_256
        canvas = torch.zeros_like(stitch)
        alpha = torch.zeros_like(full_alpha)
        canvas[:, :, y0:y1, x0:x1] = _aa_resize(stitch, 128)
        alpha[:, :, y0:y1, x0:x1] = _aa_resize(full_alpha, 128)
        planes = static_plane.clone()
        planes[:, 0] = canvas * alpha + static_plane[:, 0] * (1 - alpha)
        return planes

    def _planes(self, ws, texture_feats, static_feats, mesh_condition, update_emas, synthesis_kwargs, all_levels=False, mouth=None,
                face_head=None, pending=None):
        static_for_raster, static_plane = self._split_static(static_feats)
        assert len(static_for_raster) == len(texture_feats), (len(static_for_raster), len(texture_feats))
        if pending is not None and not all_levels:
            # The rasteriser runs on a stream of its own: level k is launched there as soon as the events of the taps it reads exist
            # (taps 0 and 1 are both 32^2 and come with the first event), under the face backbone's previous block; the face
            # backbone only waits for level k's event when it reads cond_list[k].
            main = torch.cuda.current_stream(ws.device)
            rs = _state(self).stream('raster', ws.device)
            rs.wait_stream(main)
            levels, done = [], []
            with torch.cuda.stream(rs):
                prep = self._raster_prep(mesh_condition['uvcoords_image'], mouth)      # (joins the mouth fill on this stream)
                for k in range(N_COND_LEVELS_USED):
                    need = max(2, k + 1)
                    rs.wait_event(pending[2][need])
                    rs.wait_event(pending[3][need])
                    levels.append(self._raster_level(k, texture_feats[k], static_for_raster[k], BBOX_256, prep))
                    ev = torch.cuda.Event()
                    ev.record(rs)
                    done.append(ev)
            full_alpha = prep['full_alpha']
            for t in levels:
                t.record_stream(main)

            def level(k):
                main.wait_event(done[k])
                return levels[k]
            cond = _LazyLevels(N_COND_LEVELS_USED, level)
        else:
            if pending is not None:
                for st in pending[:2]:
                    torch.cuda.current_stream(ws.device).wait_stream(st)
            cond, full_alpha, _ = self.rasterize(texture_feats, mesh_condition['uvcoords_image'], static_for_raster, BBOX_256,
                                                 levels=None if all_levels else N_COND_LEVELS_USED, _mouth=mouth)
        head = None
        if face_head is not None:
            torch.cuda.current_stream(ws.device).wait_event(face_head[3])
            head = face_head[:3]
        stitch = self.face_backbone.synthesis(ws, cond, return_list=False, update_emas=update_emas, _head=head, **synthesis_kwargs)
        if pending is not None:      # the static backbone's 256^2 taps (the planes) are consumed from here on
            torch.cuda.current_stream(ws.device).wait_stream(pending[1])
        return self._blend_planes(stitch, full_alpha, static_plane)

    def _sr_input_consumer(self, ws, nrr):
        """(layer, styles [B,32], planes) of the convolution that reads the rendered features in split format -- block0.conv0 of a two-block
        head fed at its own input resolution, with its styles parked by the frame-level style batch -- or (None, None, 0)."""
        from ..training import networks_stylegan2 as sg2
        sr = self.superresolution
        block0 = getattr(sr, 'block0', None)
        conv0 = getattr(block0, 'conv0', None)
        if (not isinstance(block0, sg2.SynthesisBlock) or conv0 is None or conv0._pre is None or getattr(sr, 'input_resolution', None) != nrr
                or conv0.in_channels != 32 or block0.architecture == 'resnet' or self.rendering_kwargs.get('superresolution_noise_mode') == 'random'):
            return None, None, 0
        half = block0._half_ops(ws.device)
        if not conv0._takes_split_input(nrr, self.rendering_kwargs.get('superresolution_noise_mode', 'const'), half):
            return None, None, 0
        styles = conv0._pre[0]
        if styles.shape != (ws.shape[0], 32) or styles.dtype != torch.float32 or not styles.is_contiguous():
            return None, None, 0
        return conv0, styles, (1 if half else 2)

    def _render(self, ws, planes, origins, dirs, nrr, evaluation, jitter, synthesis_kwargs, ray_dist=None, u_importance=None):
        if evaluation:
            assert synthesis_kwargs.get('noise_mode') == 'const', ('noise_mode' in synthesis_kwargs, synthesis_kwargs.get('noise_mode'))
        # The head's first convolution reads the features as fp16 planes multiplied by its styles (hipops.SplitAct): when those styles
        # exist already (computed at the top of the frame) the renderer writes that copy itself -- no ia_act_split launch between the
        # renderer and the head (r06; the bits of ia_act_split on the stored image)
        split_kw, consumer = {}, None
        if RENDER_WRITES_SR_INPUT and planes.is_cuda and not torch.is_grad_enabled():
            consumer, styles, n_planes = self._sr_input_consumer(ws, nrr)
            if consumer is not None:
                split_kw = dict(split_styles=styles, split_planes=n_planes)
        feats, depth, _ = self.renderer(planes, self.decoder, origins, dirs, self.rendering_kwargs, evaluation=evaluation, jitter=jitter,
                                        dist=ray_dist, **({} if u_importance is None else {'u_importance': u_importance}), **split_kw)
        n = ws.shape[0]
        feature_image = feats.permute(0, 2, 1).reshape(n, feats.shape[-1], nrr, nrr).contiguous()
        split_data = getattr(feats, 'split_data', None)
        if consumer is not None and split_data is not None:
            feature_image._ia_split = hipops.SplitAct(split_data.reshape(n, split_data.shape[1], 4, nrr, nrr, 8), feats.shape[-1], consumer)
        depth_image = depth.permute(0, 2, 1).reshape(n, 1, nrr, nrr)
        rgb = feature_image[:, :3]
        sr_kwargs = {k: v for k, v in synthesis_kwargs.items() if k != 'noise_mode'}
        image = self.superresolution(rgb, feature_image, ws, noise_mode=self.rendering_kwargs['superresolution_noise_mode'], **sr_kwargs)
        return image, rgb, depth_image, feature_image

    # ------------------------------------------------------------------ public synthesis entry points
    def synthesis(self, ws, c, mesh_condition, neural_rendering_resolution=None, update_emas=False, cache_backbone=False,
                  use_cached_backbone=False, return_featmap=False, evaluation=False, jitter=None, ray_dist=None, **synthesis_kwargs):
        side = {}
        sr_ready = self._frame_styles(ws)
        side_work = {'m': lambda: side.__setitem__('m', self._start_mouth_fill(mesh_condition, rays=(c, neural_rendering_resolution, ray_dist))),
                     'f': lambda: side.__setitem__('f', self._start_face_head(ws, update_emas, synthesis_kwargs, sr_ready))}
        texture_feats, static_feats, pending = self._two_backbones(ws, update_emas, synthesis_kwargs, partial=True,
                                                                   order=LAUNCH_ORDER, side_work=side_work)
        mouth, face_head = side['m'], side['f']
        side_rays = _state(self).side_rays
        if side_rays is not None:            # made on the side stream; joined with the mouth fill inside rasterize()
            origins, dirs, nrr, ray_dist = side_rays
        else:
            origins, dirs, nrr = self._rays(c, neural_rendering_resolution)
        planes = self._planes(ws, texture_feats, static_feats, mesh_condition, update_emas, synthesis_kwargs, mouth=mouth,
                              face_head=face_head, pending=pending)
        image, rgb, depth, feature_image = self._render(ws, planes, origins, dirs, nrr, evaluation, jitter, synthesis_kwargs, ray_dist)
        if pending is not None:      # the texture backbone's 256^2 block (not consumed by this frame's image) ends with the frame
            torch.cuda.current_stream(ws.device).wait_stream(pending[0])
        out = {'image': image, 'image_raw': rgb, 'image_depth': depth}
        if return_featmap:
            out.update(feature_image=feature_image, triplane=planes, texture=texture_feats)
        return out

    def synthesis_withTexture(self, ws, texture_feats, c, mesh_condition, static_feats=None, neural_rendering_resolution=None,
                              update_emas=False, cache_backbone=False, use_cached_backbone=False, evaluation=False, jitter=None,
                              ray_dist=None, u_importance=None, **synthesis_kwargs):
        # same orchestration as synthesis(): mouth fill + rays on the side stream, face-backbone head on its own stream
        # (`jitter`, `u_importance`: the renderer's two random draws handed in, see ImportanceRenderer_bsMotion.forward)
        # (`ray_dist`: see ImportanceRenderer_bsMotion.forward -- 1 value for the batch or one per frame)
        mouth = self._start_mouth_fill(mesh_condition, rays=(c, neural_rendering_resolution, ray_dist))
        face_head = self._start_face_head(ws, update_emas, synthesis_kwargs)
        side_rays = _state(self).side_rays
        if side_rays is not None:
            origins, dirs, nrr, ray_dist = side_rays
        else:
            origins, dirs, nrr = self._rays(c, neural_rendering_resolution)
        if static_feats is None:
            static_feats = self.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **synthesis_kwargs)
        planes = self._planes(ws, texture_feats, static_feats, mesh_condition, update_emas, synthesis_kwargs, mouth=mouth,
                              face_head=face_head)
        image, rgb, depth, feature_image = self._render(ws, planes, origins, dirs, nrr, evaluation, jitter, synthesis_kwargs, ray_dist, u_importance)
        return {'image': image, 'image_raw': rgb, 'image_depth': depth, 'feature_image': feature_image, 'triplane': planes}

    def synthesis_withCondition(self, ws, c, mesh_condition, gt_texture_feats=None, gt_static_feats=None, texture_feats_conditions=None,
                                static_feats_conditions=None, neural_rendering_resolution=None, update_emas=False, cache_backbone=False,
                                use_cached_backbone=False, only_image=False, return_feats=False, jitter=None, **synthesis_kwargs):
        origins, dirs, nrr = self._rays(c, neural_rendering_resolution)
        texture_feats = gt_texture_feats
        if texture_feats is None:
            texture_feats = self.texture_backbone.synthesis(ws, cond_list=None, return_list=True, feat_conditions=texture_feats_conditions,
                                                            update_emas=update_emas, **synthesis_kwargs)
        static_feats = gt_static_feats
        if static_feats is None:
            static_feats = self.backbone.synthesis(ws, cond_list=None, return_list=True, feat_conditions=static_feats_conditions,
                                                   update_emas=update_emas, **synthesis_kwargs)
        planes = self._planes(ws, texture_feats, static_feats, mesh_condition, update_emas, synthesis_kwargs)
        evaluation = synthesis_kwargs.get('noise_mode') == 'const'
        image, rgb, depth, feature_image = self._render(ws, planes, origins, dirs, nrr, evaluation, jitter, synthesis_kwargs)
        if only_image:
            return {'image': image}
        out = {'image': image, 'image_raw': rgb, 'image_depth': depth, 'feature_image': feature_image, 'triplane': planes}
        if return_feats:
            out['static'] = static_feats
            out['texture'] = texture_feats
        return out

    def rasterize(self, texture_feats, uvcoords_image, static_feats, bbox_256, levels=None, _mouth=None):
        """UV-rasterise the neural texture pyramid and blend it over the static features.

        uvcoords_image [B,H,W,3] = (u, v, mask).  Returns (list of [B, C_k+1, res_k, res_k], full_alpha, mouth_masks);
        the extra channel is the face alpha with the upper part of the mouth hole closed (:324-326).
        `levels` limits how many pyramid levels are produced (None = all, as the reference)."""
        prep = self._raster_prep(uvcoords_image, _mouth)
        n = len(texture_feats) if levels is None else min(levels, len(texture_feats))
        out = [self._raster_level(k, tex, sta, bbox_256, prep) for k, (tex, sta) in enumerate(zip(texture_feats[:n], static_feats[:n]))]
        return out, prep['full_alpha'], prep['mouth']

    def _raster_prep(self, uvcoords_image, _mouth=None):
        """Per-frame inputs of the rasteriser: UV grid, face alpha, filled mouth (joined here if it was started on the side stream)."""
        uv = uvcoords_image if uvcoords_image.dtype == torch.float32 else uvcoords_image.float()
        grid, alpha = uv[..., :2], uv[..., 2:].permute(0, 3, 1, 2)
        fused = uv.is_cuda and uv.shape[1:3] == (256, 256) and not torch.is_grad_enabled()
        uv_c = upper_c = None
        if _mouth is not None:   # started on the side stream by synthesis(): join it here
            alpha, full_alpha, mouth, done, uv_c, upper_c = _mouth
            torch.cuda.current_stream(uv.device).wait_event(done)
            upper_alpha = upper_c.unsqueeze(1)
        else:
            full_alpha, mouth = fill_mouth(alpha.clone(), blur_mouth_edge=False)
            upper_alpha = self._upper_alpha(alpha, mouth)
            if fused:
                uv_c, upper_c = uv.contiguous(), upper_alpha.reshape(-1, 256, 256).contiguous()
        # channels-last copies made on the texture stream by _two_backbones (same list object => same frame)
        st = _state(self)
        cached, st.tex_cl = st.tex_cl, None
        return dict(grid=grid, alpha=alpha, full_alpha=full_alpha, mouth=mouth, upper_alpha=upper_alpha, uv_c=uv_c, upper_c=upper_c,
                    fused=fused, cached=cached)

    def _raster_level(self, k, tex, sta, bbox_256, prep):
        """One pyramid level: texture sampled through the UV map, AA-resized, blended over the static features' bbox crop."""
        res = tex.shape[2]
        y0, y1, x0, x1 = [round(v * res / 256) for v in bbox_256]
        if prep['fused'] and res in (32, 64, 128) and tex.dtype == torch.float32 and sta.dtype == torch.float32:
            cached = prep['cached']
            cl = cached[1][k] if (cached is not None and k < len(cached[0]) and cached[0][k] is tex and k < len(cached[1])) else None
            return hipops.rasterize_level(tex, prep['uv_c'], prep['upper_c'], sta, (y0, y1, x0, x1), res, tex_cl=cl)
        rend = _aa_resize(F.grid_sample(tex, prep['grid'], align_corners=False), res)
        a = _aa_resize(prep['alpha'], res)
        s = _aa_resize(sta[:, :, y0:y1, x0:x1], res)
        return torch.cat([rend * a + s * (1 - a), _aa_resize(prep['upper_alpha'], res)], dim=1)

    def visualize_mesh_condition(self, mesh_condition, to_imgs=False):
        uv = mesh_condition['uvcoords_image'].clone().permute(0, 3, 1, 2)
        full_alpha, _ = fill_mouth(uv[:, 2:].clone(), blur_mouth_edge=False)
        if not to_imgs:
            return uv
        uv[full_alpha.expand(-1, 3, -1, -1) == 0] = -1
        return [img for img in ((uv + 1) * 127.5).to(dtype=torch.uint8).cpu()]   # uint8 CHW tensors (no torchvision here)

    # ------------------------------------------------------------------ point queries (shape extraction)
    def _query(self, ws, coordinates, directions, mesh_condition, update_emas, synthesis_kwargs):
        texture_feats = self.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **synthesis_kwargs)
        static_feats = self.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **synthesis_kwargs)
        planes = self._planes(ws, texture_feats, static_feats, mesh_condition, update_emas, synthesis_kwargs)
        self.renderer.plane_axes = self.renderer.plane_axes.to(planes.device)
        return self.renderer.run_model(planes, self.decoder, coordinates, directions, self.rendering_kwargs)

    def sample(self, coordinates, directions, z, c, mesh_condition, truncation_psi=1, truncation_cutoff=None, update_emas=False,
               **synthesis_kwargs):
        ws = self.mapping(z, c, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, update_emas=update_emas)
        return self._query(ws, coordinates, directions, mesh_condition, update_emas, synthesis_kwargs)

    def sample_mixed(self, coordinates, directions, ws, mesh_condition, truncation_psi=1, truncation_cutoff=None, update_emas=False,
                     **synthesis_kwargs):
        return self._query(ws, coordinates, directions, mesh_condition, update_emas, synthesis_kwargs)

    def query_points(self, ws, coordinates, mesh_condition, **synthesis_kwargs):
        """What ``sample_mixed`` returns ({'rgb' [B,M,32], 'sigma' [B,M,1]}) without ray directions (the decoder ignores them).  Device
        tensors: the planes, then ONE ``ia_query_planes`` launch (gather + decoder, fp32) instead of grid_sample + two linear layers."""
        from .. import geometry
        planes = geometry.generator_planes(self, ws, mesh_condition, **synthesis_kwargs)
        return geometry.query_planes(planes, self.decoder, coordinates, self.rendering_kwargs['box_warp'], rgb=True)

    @torch.no_grad()
    def extract_geometry(self, ws, mesh_condition, resolution=256, level=10.0, cube_length=None, origin=(0, 0, 0), with_colors=False,
                         with_normals=False, keep=None, min_voxels=0, simplify=None, smooth=None, texture=None, fit_template=None,
                         **synthesis_kwargs):
        """Shape of the avatar: one dict per batch element with 'volume' [N,N,N] (density on the lattice of
        ``invertavatar_amd.geometry``: ``cube_length`` (default: box_warp) around ``origin``), 'verts' float32 [V,3] (same coordinates
        as the queries), 'faces' int64 [F,3] (outward-wound marching-cubes mesh of density > ``level``) and, with ``with_colors``,
        'colors' uint8 [V,3] (the decoder's rgb[:3] at the vertices) and, with ``with_normals``, 'normals' float32 [V,3]
        (``geometry.volume_normals``: unit, toward decreasing density).  ``level`` = 10 is the EG3D-family shape threshold: a knob, not a
        constant of the model.  With ``keep`` (``'largest'``, an int n or a list of labels; ``min_voxels``: see
        ``geometry.select_components``) the detached components of {density > level} are removed from the volume first
        (``geometry.keep_components``, 26-connectivity): 'volume' is then the filtered volume, mesh, colours and normals come from it, and
        'components' holds {'count', 'kept', 'stats'}.  ``simplify`` (None: nothing changes; an int = ``target_faces``; or a dict of
        ``geometry.simplify_mesh`` keyword arguments) simplifies the mesh after the filter and marching cubes: 'verts' and 'faces' are
        then the simplified mesh, colours and normals are queried at its vertices (exact there, and cheaper than averaging), and
        'simplify' holds {'dims', 'cell_size', 'faces_before', 'faces_after', 'verts_before', 'verts_after'} (and 'steps' with a
        target).  ``smooth`` (None: nothing changes; an int = Taubin pairs with the defaults of ``geometry.smooth_mesh``; or a dict of
        its keyword arguments) smooths the mesh after the filter and after ``simplify``: 'faces' stay, 'verts' move, colours are
        queried at the final vertices, normals come from the mesh (``geometry.mesh_normals``) instead of the volume, and 'smooth' holds
        the smoothing's 'info' ('edges', 'boundary_edges', 'nonmanifold_edges', 'steps', ...).  ``texture`` (None: nothing changes; an
        int = the atlas size with the decoder as source; or a dict of ``bake_texture`` keyword arguments) bakes the colours of the
        FINAL mesh (after ``keep``, ``simplify`` and ``smooth``) into a texture atlas: 'texture' [size,size,3], 'uv' float32 [F,3,2],
        'atlas' and 'texture_info' {'filled', 'mask' and, from views, 'views'}.  ``fit_template`` (None: nothing changes; a ``(verts,
        faces)`` pair; or a dict with 'verts', 'faces', optionally 'align' (``'rigid'`` or ``'similarity'``: ``geometry.align_mesh`` from
        ``init='centroid'`` first, or with 'align_init': 'global' from a pose search) and ``geometry.nonrigid_align`` keyword arguments) wraps that template onto the FINAL mesh: 'template'
        holds {'verts' (the template's vertices on the avatar's shape), 'faces' (the template's own), 'fit' (``nonrigid_align``'s result),
        with ``with_colors`` 'colors' (queried at the fitted vertices) and with 'align' 'alignment' (``align_mesh``'s result)}: one fixed
        topology for every seed.  The planes are computed once per call; device tensors stay on the device throughout."""
        from .. import geometry
        box_warp = self.rendering_kwargs['box_warp']
        length = box_warp if cube_length is None else cube_length
        planes = geometry.generator_planes(self, ws, mesh_condition, **synthesis_kwargs)
        volume = geometry.density_volume(planes, self.decoder, resolution, length, origin, box_warp)
        res, ls, org = geometry._res3(resolution), geometry._vec3(length), geometry._vec3(origin)
        axes = [geometry.lattice_axis(n, ls[a], org[a]) for a, n in enumerate(res)]
        out = []
        for b in range(volume.shape[0]):
            vol_b, info = volume[b], None
            if keep is not None:
                vol_b, info = geometry.keep_components(vol_b, level, keep, min_voxels)
            verts, faces = geometry.marching_cubes(vol_b, level, [float(a[1]) for a in axes], [float(a[2]) for a in axes])
            item = {'volume': vol_b, 'verts': verts, 'faces': faces}
            if info is not None:
                item['components'] = info
            if simplify is not None:
                kw = dict(simplify) if isinstance(simplify, dict) else {'target_faces': int(simplify)}
                simple = geometry.simplify_mesh(verts, faces, **kw)
                item['simplify'] = {'dims': simple['dims'], 'cell_size': simple['cell_size'], 'faces_before': int(faces.shape[0]),
                                    'faces_after': int(simple['faces'].shape[0]), 'verts_before': int(verts.shape[0]),
                                    'verts_after': int(simple['verts'].shape[0]), **({'steps': simple['steps']} if 'steps' in simple else {})}
                verts, faces = simple['verts'], simple['faces']
                item['verts'], item['faces'] = verts, faces
            adjacency = None
            if smooth is not None:
                kw = dict(smooth) if isinstance(smooth, dict) else {'iterations': int(smooth)}
                smoothed = geometry.smooth_mesh(verts, faces, **kw)
                verts, adjacency = smoothed['verts'], smoothed['adjacency']
                item['verts'], item['smooth'] = verts, dict(smoothed['info'])
            if with_colors:
                item['colors'] = geometry.vertex_colors(planes[b:b + 1], self.decoder, verts, box_warp)
            if with_normals and smooth is not None:
                item['normals'] = geometry.mesh_normals(verts, faces, adjacency=adjacency)
            elif with_normals:
                item['normals'] = geometry.volume_normals(vol_b, verts, [float(a[1]) for a in axes], [float(a[2]) for a in axes])
            if texture is not None:
                kw = dict(texture) if isinstance(texture, dict) else {'size': int(texture)}
                cond_b = {k: x[b:b + 1] if isinstance(x, torch.Tensor) and x.shape[0] == ws.shape[0] else x for k, x in mesh_condition.items()}
                baked = self.bake_texture(ws[b:b + 1], cond_b, verts, faces, **kw, **synthesis_kwargs)
                item['texture'], item['uv'], item['atlas'] = baked['texture'], baked['uv'], baked['atlas']
                item['texture_info'] = {k: baked[k] for k in ('filled', 'mask', 'views') if k in baked}
            if fit_template is not None:
                kw = dict(fit_template) if isinstance(fit_template, dict) else {'verts': fit_template[0], 'faces': fit_template[1]}
                tv = torch.as_tensor(kw.pop('verts')).to(verts.device).float().contiguous()
                tf = torch.as_tensor(kw.pop('faces')).to(verts.device)
                how, start, wrapped = kw.pop('align', None), kw.pop('align_init', 'centroid'), {'faces': tf}
                if how is not None:
                    if how not in ('rigid', 'similarity'):
                        raise ValueError(f"fit_template['align'] must be None, 'rigid' or 'similarity', got {how!r}")
                    if start not in ('centroid', 'global'):
                        raise ValueError(f"fit_template['align_init'] must be 'centroid' or 'global', got {start!r}")
                    wrapped['alignment'] = geometry.align_mesh((tv, tf), verts, faces, scale=how == 'similarity', init=start,
                                                               **({'search': kw['search']} if 'search' in kw else {}))
                    tv = geometry.transform_points(tv, wrapped['alignment']['matrix'])
                wrapped['fit'] = geometry.nonrigid_align((tv, tf), verts, faces, **kw)
                wrapped['verts'] = wrapped['fit']['verts']
                if with_colors:
                    wrapped['colors'] = geometry.vertex_colors(planes[b:b + 1], self.decoder, wrapped['verts'], box_warp)
                item['template'] = wrapped
            out.append(item)
        return out

    @torch.no_grad()
    def render_geometry(self, ws, c, mesh_condition, resolution=512, volume_resolution=256, level=10.0, cube_length=None, with_colors=False,
                        keep=None, min_voxels=0, **synthesis_kwargs):
        """Surface renders of the avatar's shape from the cameras ``c`` ([B,25] or [B,V,25]): per identity the density volume of
        ``extract_geometry`` (``volume_resolution``^3 over ``cube_length``, default box_warp) and the first hit of every camera ray
        (``geometry.raycast``; rays of the generator's ray sampler, so pixels align with ``image_depth`` at the same resolution) with
        {density > level}, all views of an identity in one launch.  Returns NCHW 'depth' [B(,V),1,H,W] (ray parameter; 0 on a miss),
        'mask' bool [B(,V),1,H,W], 'normal' [B(,V),3,H,W] (unit, toward decreasing density), 'shaded' [B(,V),1,H,W] (headlight
        Lambert, ``geometry.shade``) and, with ``with_colors``, 'rgb' [B(,V),3,H,W] (the decoder's rgb[:3] at the hit points, 0 on a
        miss).  ``keep`` / ``min_voxels``: as in ``extract_geometry``, the volume is filtered before the bricks and the ray cast."""
        from .. import geometry
        single = c.dim() == 2
        cams = c[:, None] if single else c
        B, V = cams.shape[:2]
        if ws.shape[0] != B:
            raise ValueError(f'ws has batch {ws.shape[0]} but c has {B}')
        box_warp = self.rendering_kwargs['box_warp']
        length = box_warp if cube_length is None else cube_length
        planes = geometry.generator_planes(self, ws, mesh_condition, **synthesis_kwargs)
        volume = geometry.density_volume(planes, self.decoder, volume_resolution, length, (0, 0, 0), box_warp)
        res, ls = geometry._res3(volume_resolution), geometry._vec3(length)
        axes = [geometry.lattice_axis(n, ls[a], 0.0) for a, n in enumerate(res)]
        lo, step = [float(a[1]) for a in axes], [float(a[2]) for a in axes]
        cam = cams.reshape(B * V, 25).float()
        rays_o, rays_d = self.ray_sampler(cam[:, :16].view(-1, 4, 4), cam[:, 16:25].view(-1, 3, 3), resolution)
        rays_o, rays_d = rays_o.reshape(B, V * resolution * resolution, 3), rays_d.reshape(B, V * resolution * resolution, 3)
        outs = []
        for b in range(B):
            vol_b = volume[b] if keep is None else geometry.keep_components(volume[b], level, keep, min_voxels)[0]
            hit = geometry.raycast(vol_b, level, lo, step, rays_o[b], rays_d[b])
            hit['shaded'] = geometry.shade(hit['normal'], rays_d[b], hit['mask'])
            if with_colors:
                pts = (rays_o[b] + hit['depth'][:, None] * rays_d[b])[None]
                rgb = geometry.query_planes(planes[b:b + 1], self.decoder, pts, box_warp, rgb=True)['rgb'][0, :, :3]
                hit['rgb'] = rgb * hit['mask'][:, None]
            outs.append(hit)
        lead = (B,) if single else (B, V)
        out = {}
        for k in outs[0]:
            x = torch.stack([o[k] for o in outs])
            x = x.reshape(B * V, resolution, resolution, -1).permute(0, 3, 1, 2)
            out[k] = x.reshape(lead + x.shape[1:])
        return out

    def render_mesh(self, verts, faces, c, resolution=512, normals=None, colors=None, cull='none', texture=None, atlas=None):
        """Renders of one triangle mesh (verts [V,3], faces [F,3]: an extracted, simplified or smoothed mesh, or one read with
        ``read_ply``) from the cameras ``c`` ([V,25] or [B,V,25]) through ``geometry.rasterize_mesh``; pixels align with
        ``render_geometry`` and ``image_depth`` at the same resolution.  Returns the NCHW dictionary of ``render_geometry``: 'depth'
        [(B,)V,1,H,W] (ray parameter; 0 on a miss), 'mask' bool, 'normal' [(B,)V,3,H,W] (the face normal of the winding, or with
        ``normals`` [V,3] their interpolation), 'shaded' (headlight Lambert, ``geometry.shade`` with the rays of the generator's ray
        sampler) and, with ``colors`` ([V,3], uint8 or float in [0, 1]), 'rgb' [(B,)V,3,H,W] (0 on a miss); besides these 'culled'
        int32 [(B,)V], the triangles dropped per view for a vertex at or behind the near plane (nothing is clipped).  With ``texture``
        [size,size,C] and its ``atlas`` (``geometry.TextureAtlas``) 'rgb' [(B,)V,C,H,W] is ``geometry.sample_texture`` of the raster's
        face and barycentrics instead of the interpolated vertex colours."""
        from .. import geometry
        if (texture is None) != (atlas is None):
            raise ValueError('texture and atlas are given together')
        lead = tuple(c.shape[:-1])
        cam = c.reshape(-1, 25).float()
        attrs = None
        if colors is not None:
            attrs = colors.float() / 255 if colors.dtype == torch.uint8 else colors.float()
        hit = geometry.rasterize_mesh(verts, faces, cam, resolution, normals=normals, attributes=attrs, cull=cull)
        _, rays_d = self.ray_sampler(cam[:, :16].view(-1, 4, 4), cam[:, 16:25].view(-1, 3, 3), resolution)
        rays_d = rays_d.reshape(-1, resolution, resolution, 3)
        out = {'depth': hit['depth'][..., None], 'mask': hit['mask'][..., None], 'normal': hit['normal'],
               'shaded': geometry.shade(hit['normal'], rays_d, hit['mask'])}
        if colors is not None:
            out['rgb'] = hit['attributes']
        if texture is not None:
            out['rgb'] = geometry.sample_texture(texture, atlas, hit['face'], hit['bary'])
        out = {k: x.permute(0, 3, 1, 2).reshape(lead + (x.shape[3], resolution, resolution)) for k, x in out.items()}
        out['culled'] = hit['culled'].reshape(lead)
        return out

    @torch.no_grad()
    def bake_texture(self, ws, mesh_condition, verts, faces, size=2048, source='decoder', cameras=None, mode='blend', n_views=8, atlas=None,
                     **synthesis_kwargs):
        """The colours of the avatar ``ws`` [1,L,512] on the texture atlas of a mesh of it (verts [V,3], faces [F,3]: the output of
        ``extract_geometry``).  ``source='decoder'``: the decoder's rgb[:3] at the surface point of every texel
        (``geometry.bake_colors``).  ``source='views'``: ``synthesis(ws, c, mesh_condition)['image']`` of every camera of ``cameras``
        [N,25] (default: the yaw orbit of ``extract_geometry.orbit_cameras`` with ``n_views`` views), mapped to [0, 1] and projected
        onto the mesh (``geometry.project_texture``, ``mode``) with the decoder bake as the fallback of the texels no view sees.  Returns
        {'texture' [size,size,3], 'atlas', 'uv' float32 [F,3,2], 'mask' (owned texels), 'filled', 'views' (int32, views per texel),
        'weight'}; for the decoder source 'filled' is 'mask' and 'views' / 'weight' are absent."""
        from .. import geometry
        if source not in ('decoder', 'views'):
            raise ValueError(f"source must be 'decoder' or 'views', got {source!r}")
        if ws.shape[0] != 1:
            raise ValueError(f'bake_texture takes one avatar, got a batch of {ws.shape[0]}')
        box_warp = self.rendering_kwargs['box_warp']
        planes = geometry.generator_planes(self, ws, mesh_condition, **synthesis_kwargs)
        atlas = geometry.TextureAtlas(int(faces.shape[0]), size) if atlas is None else atlas
        dec = geometry.bake_colors(planes[:1], self.decoder, verts, faces, size, box_warp, atlas=atlas)
        out = {'texture': dec['texture'], 'atlas': atlas, 'uv': atlas.uv, 'mask': dec['mask'], 'filled': dec['mask']}
        if source == 'decoder':
            return out
        if cameras is None:
            from ..extract_geometry import orbit_cameras
            cameras = orbit_cameras(self, n_views, device=ws.device)
        cameras = cameras.reshape(-1, 25).float()
        images = torch.cat([self.synthesis(ws, cameras[k:k + 1], mesh_condition, **synthesis_kwargs)['image'] for k in range(cameras.shape[0])])
        images = ((images.float() + 1) / 2).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
        proj = geometry.project_texture(verts, faces, atlas, images, cameras, mode=mode, fallback=dec['texture'])
        out.update(texture=proj['texture'], filled=proj['filled'], views=proj['views'], weight=proj['weight'])
        return out

    def forward(self, z, c, v, truncation_psi=1, truncation_cutoff=None, neural_rendering_resolution=None, update_emas=False,
                cache_backbone=False, use_cached_backbone=False, **synthesis_kwargs):
        ws = self.mapping(z, c, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, update_emas=update_emas)
        return self.synthesis(ws, c, v, update_emas=update_emas, neural_rendering_resolution=neural_rendering_resolution,
                              cache_backbone=cache_backbone, use_cached_backbone=use_cached_backbone, **synthesis_kwargs)


class OSGDecoder(torch.nn.Module):
    """Tiny MLP that decodes averaged tri-plane features into density + 32 colour channels (:415-438).
    Inside ``ia_render_rays`` its two layers run on MFMA; this module form serves CPU tensors and point queries."""

    def __init__(self, n_features, options):
        super().__init__()
        self.hidden_dim = 64
        self.net = torch.nn.Sequential(
            FullyConnectedLayer(n_features, self.hidden_dim, lr_multiplier=options['decoder_lr_mul']),
            torch.nn.Softplus(),
            FullyConnectedLayer(self.hidden_dim, 1 + options['decoder_output_dim'], lr_multiplier=options['decoder_lr_mul']))

    def forward(self, sampled_features, ray_directions, sampled_embeddings=None):
        x = sampled_features.mean(1)
        n, m, c = x.shape
        x = self.net(x.view(n * m, c)).view(n, m, -1)
        rgb = torch.sigmoid(x[..., 1:]) * (1 + 2 * 0.001) - 0.001   # MipNeRF sigmoid clamping
        return {'rgb': rgb, 'sigma': x[..., 0:1]}
