"""SD finetune trainer — the reference's diff_train hot loop, MI355X-native.

Loop semantics parity (/root/reference/diff_train.py:613-733):
VAE encode ×0.18215 → per-sample timesteps → add_noise → text encode →
embedding mitigations (gaussian noise / mixup) → UNet forward → target
(epsilon | v_prediction) → fp32 MSE → backward (overlapped bucketed RCCL
all-reduce) → clip grad 1.0 → fused AdamW → lr schedule → {loss, lr} log →
periodic sample grids + diffusers-layout checkpoints.

MI355X design deltas vs the reference:
* FusedAdamW flat-buffer optimizer (one HIP kernel per step) instead of
  ~700 per-tensor torch.optim launches.
* GradBucketAllReduce hooks launch per-bucket RCCL all-reduce during
  backward (xGMI overlap) instead of accelerate's DDP wrapper.
* bf16 autocast compute; GroupNorm+SiLU / LayerNorm / GEGLU / attention
  are hand-written CDNA4 kernels (dcr_amd.ops).
* checkpoint_{step}/ additionally contains state.pt so training can
  RESUME (the reference cannot — SURVEY.md §5.4).
"""
from __future__ import annotations

import os
import random
import time
from pathlib import Path
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, WeightedRandomSampler
from torch.utils.data.distributed import DistributedSampler

from ..data import (HashTokenizer, ObjectAttributeDataset, SyntheticImageDataset,
                    collate_fn, load_tokenizer)
from ..models import (AutoencoderKL, CLIPTextModel, UNet2DConditionModel,
                      UNetConfig, model_configs)
from ..models.model_io import save_pipeline_index
from ..ops.adamw import FusedAdamW
from ..parallel import GradBucketAllReduce, dist as dist_utils
from ..schedulers import DDPMScheduler
from ..utils import Tracker
from ..utils.profiler import PhaseProfiler
from .config import TrainConfig, get_lr


def set_seed(seed: int):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class Trainer:
    def __init__(self, cfg: TrainConfig, device: Optional[torch.device] = None):
        self.cfg = cfg
        self.rank = dist_utils.get_rank()
        self.world = dist_utils.get_world_size()
        if device is None:
            device = torch.device("cuda", dist_utils.get_local_rank()) \
                if torch.cuda.is_available() else torch.device("cpu")
        self.device = device
        if self.device.type == "cuda":
            # MIOpen exhaustive find on first occurrence of each conv shape:
            # measured +33% step throughput vs FAST find mode on MI355X
            # (profiles/r01: workspace-limited fallback solvers otherwise).
            torch.backends.cudnn.benchmark = True
        if cfg.seed is not None:
            set_seed(cfg.seed + self.rank)

        self.weight_dtype = {
            "no": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16,
            "pure_bf16": torch.bfloat16,
        }[cfg.mixed_precision]
        self.pure_bf16 = cfg.mixed_precision == "pure_bf16"
        # fp16 needs loss scaling (reference parity: utils_ret.py:834-860);
        # bf16 does not.
        self.scaler = torch.amp.GradScaler("cuda") \
            if cfg.mixed_precision == "fp16" and torch.cuda.is_available() else None
        self._finite_streak = 0  # consecutive finite fp16 steps (manual growth)

        self._build_models()
        self._build_data()
        self._build_optimizer()

        self.noise_scheduler = DDPMScheduler(
            prediction_type=cfg.prediction_type or "epsilon")
        self._ac_dev = self.noise_scheduler.alphas_cumprod.to(self.device)

        self.global_step = 0
        self.tracker = None
        self.prof = PhaseProfiler()  # enabled via DCR_PROFILE=1
        self._graph = None  # hipGraph-captured step (enable_hipgraph)

    # ------------------------------------------------------------------
    def _build_models(self):
        cfg = self.cfg
        pretrained = Path(cfg.pretrained_model_name_or_path)
        if (pretrained / "model_index.json").exists():
            # local diffusers-layout checkpoint (checkpoint/ or checkpoint_{N}/)
            self.unet = UNet2DConditionModel.from_pretrained(pretrained / "unet")
            self.vae = AutoencoderKL.from_pretrained(pretrained / "vae")
            self.text_encoder = CLIPTextModel.from_pretrained(pretrained / "text_encoder")
            self.tokenizer = load_tokenizer(pretrained / "tokenizer")
        else:
            # no network: random-init models of the named architecture
            ucfg, vcfg, tcfg = model_configs(cfg.model_size)
            if cfg.unet_from_scratch == "yes" and cfg.unet_config:
                ucfg = UNetConfig.from_json(Path(cfg.unet_config).read_text())
            self.unet = UNet2DConditionModel(ucfg)
            self.vae = AutoencoderKL(vcfg)
            self.text_encoder = CLIPTextModel(tcfg)
            self.tokenizer = HashTokenizer()
        if cfg.tokenizer_name:
            # reference diff_train.py:371-374: explicit tokenizer dir wins
            self.tokenizer = load_tokenizer(cfg.tokenizer_name)

        self.vae.requires_grad_(False)
        if not self.cfg.train_text_encoder:
            self.text_encoder.requires_grad_(False)

        self.unet.to(self.device,
                     dtype=torch.bfloat16 if self.pure_bf16 else None)
        if self.cfg.channels_last and self.device.type == "cuda":
            self.unet.to(memory_format=torch.channels_last)
            self.vae.to(memory_format=torch.channels_last)
        # frozen models run in the compute dtype (reference: diff_train.py:531-533)
        self.vae.to(self.device, dtype=self.weight_dtype)
        self.text_encoder.to(
            self.device,
            dtype=self.weight_dtype if not self.cfg.train_text_encoder else None)
        self.vae.eval()
        if not self.cfg.train_text_encoder:
            self.text_encoder.eval()

        if self.cfg.gradient_checkpointing:
            self._enable_grad_ckpt()

    def _enable_grad_ckpt(self):
        # wrap pure submodules (resnets/attentions) — whole up/down blocks
        # mutate the skip-connection list, which breaks checkpoint replay
        from torch.utils.checkpoint import checkpoint
        from ..models.attention import Transformer2DModel
        from ..models.resnet import ResnetBlock2D

        for mod in self.unet.modules():
            if isinstance(mod, (ResnetBlock2D, Transformer2DModel)):
                orig = mod.forward

                def wrapped(*args, _orig=orig, **kw):
                    return checkpoint(_orig, *args, use_reentrant=False, **kw)

                mod.forward = wrapped

    def _build_data(self):
        cfg = self.cfg
        if cfg.synthetic_data or cfg.instance_data_dir is None:
            self.dataset = SyntheticImageDataset(
                cfg.synthetic_size, cfg.resolution, self.tokenizer,
                seed=cfg.seed or 0)
            weights = None
        else:
            self.dataset = ObjectAttributeDataset(
                cfg.instance_data_dir, self.tokenizer,
                class_prompt=cfg.class_prompt, size=cfg.resolution,
                center_crop=cfg.center_crop, random_flip=cfg.random_flip,
                prompt_json=cfg.prompt_json, duplication=cfg.duplication,
                trainspecial=cfg.trainspecial, trainspecial_prob=cfg.trainspecial_prob,
                weight_pc=cfg.weight_pc, dup_weight=cfg.dup_weight, seed=cfg.seed)
            weights = getattr(self.dataset, "samplingweights", None)

        # trainsubset: fraction of the dataset (reference diff_train.py:466-468)
        if cfg.trainsubset is not None and cfg.trainsubset > 0:
            n_keep = int(len(self.dataset) * float(cfg.trainsubset))
            base = self.dataset
            self.dataset = torch.utils.data.Subset(base, list(range(n_keep)))
            # keep caption pool visible for sample prompts
            if hasattr(base, "prompts"):
                self.dataset.prompts = base.prompts
            if weights is not None:
                weights = weights[:n_keep]

        if weights is not None:
            # duplication sampling (reference: diff_train.py:470-479);
            # per-rank generator seed so ranks draw different samples
            g = torch.Generator()
            g.manual_seed((cfg.seed or 0) * 1000 + self.rank)
            sampler = WeightedRandomSampler(weights, len(weights), generator=g)
        elif self.world > 1:
            sampler = DistributedSampler(self.dataset, num_replicas=self.world,
                                         rank=self.rank, shuffle=True, seed=cfg.seed or 0)
        else:
            sampler = None

        self.dataloader = DataLoader(
            self.dataset, batch_size=cfg.train_batch_size, sampler=sampler,
            shuffle=(sampler is None), collate_fn=collate_fn,
            num_workers=cfg.dataloader_num_workers, pin_memory=torch.cuda.is_available(),
            drop_last=True, persistent_workers=cfg.dataloader_num_workers > 0)

    def _build_optimizer(self):
        cfg = self.cfg
        lr = cfg.learning_rate
        if cfg.scale_lr:
            lr = lr * cfg.gradient_accumulation_steps * cfg.train_batch_size * self.world
        params = list(self.unet.parameters())
        if cfg.train_text_encoder:
            params += list(self.text_encoder.parameters())
        self.optimizer = FusedAdamW(
            params, lr=lr, betas=(cfg.adam_beta1, cfg.adam_beta2),
            eps=cfg.adam_epsilon, weight_decay=cfg.adam_weight_decay,
            device_state=os.environ.get("DCR_DEV_ADAMW") == "1",
            max_grad_norm=cfg.max_grad_norm,
            state_bits=8 if cfg.use_8bit_adam else 32)
        self.ddp = GradBucketAllReduce(self.optimizer, bucket_mb=cfg.ddp_bucket_mb)

    # ------------------------------------------------------------------
    # hipGraph-captured step: the whole micro-step (VAE encode, noise,
    # text encode, UNet fwd/bwd, grad gather, device-state AdamW with
    # fused clip) replays as ONE graph launch — the per-step host work
    # is two H2D batch copies and a 4-byte lr write. Philox RNG is
    # graph-safe (each replay draws fresh noise/timesteps).
    def enable_hipgraph(self, batch) -> None:
        cfg = self.cfg
        assert self.device.type == "cuda", "hipGraph capture needs a GPU"
        assert self.pure_bf16 and self.scaler is None, \
            "graph capture: pure_bf16 only (no GradScaler host branches)"
        assert cfg.gradient_accumulation_steps == 1
        assert cfg.mixup_noise_lam == 0, "mixup draws host RNG per step"
        assert self.world == 1, "multi-rank capture not enabled yet"
        assert self.optimizer.state_bits == 32, \
            "graph capture: no device-state step for 8-bit optimizer state " \
            "(use_8bit_adam)"
        if self.optimizer.hyper is None:
            # device-state mode: per-step scalars live on device so the
            # captured kernels read them indirectly (lr updated by a
            # 4-byte write OUTSIDE the graph)
            self.optimizer.hyper = torch.tensor(
                [self.optimizer.lr, 1, 1, 1, 1, 1, 0, 0],
                dtype=torch.float32, device=self.device)
        self._g_pix = batch["pixel_values"].to(self.device).clone()
        if cfg.channels_last:
            self._g_pix = self._g_pix.contiguous(
                memory_format=torch.channels_last)
        self._g_ids = batch["input_ids"].to(self.device).clone()

        self.optimizer.zero_grad()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self._capture_body()
                self.optimizer.zero_grad()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        # thread_local: only THIS thread's HIP calls are captured —
        # background threads (pinned-memory, profiler watchdogs) would
        # otherwise trip hipErrorStreamCaptureUnsupported under the
        # default global mode
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._g_loss = self._capture_body()
        self._graph = g

    def _capture_body(self) -> torch.Tensor:
        cfg = self.cfg
        with torch.no_grad():
            latents = self.vae.encode(
                self._g_pix.to(self.weight_dtype)).latent_dist.sample()
            latents = latents * self.vae.config.scaling_factor
            noise = torch.randn_like(latents)
            timesteps = torch.randint(
                0, self.noise_scheduler.num_train_timesteps,
                (latents.shape[0],), device=self.device, dtype=torch.long)
            noisy_latents = self.noise_scheduler.add_noise(
                latents, noise, timesteps)
            encoder_hidden_states = self.text_encoder(self._g_ids)[0]
        if cfg.rand_noise_lam > 0:
            encoder_hidden_states = encoder_hidden_states + \
                cfg.rand_noise_lam * torch.randn_like(encoder_hidden_states)
        model_pred = self.unet(noisy_latents, timesteps, encoder_hidden_states)
        if self.noise_scheduler.prediction_type == "epsilon":
            target = noise
        else:
            target = self.noise_scheduler.get_velocity(latents, noise, timesteps)
        loss = F.mse_loss(model_pred.float(), target.float(), reduction="mean")
        loss.backward()
        self.optimizer.gather_grads()
        self.optimizer.step_dev()  # clip fused; scalars from hyper[]
        return loss.detach()

    def _graph_replay(self, batch) -> torch.Tensor:
        cfg = self.cfg
        pix = batch["pixel_values"].to(self.device, non_blocking=True)
        if cfg.channels_last:
            pix = pix.contiguous(memory_format=torch.channels_last)
        self._g_pix.copy_(pix, non_blocking=True)
        self._g_ids.copy_(batch["input_ids"].to(self.device), non_blocking=True)
        lr_step = get_lr(cfg, self.global_step, self.world)
        if lr_step != self.optimizer.lr:
            self.optimizer.lr = lr_step
            self.optimizer.hyper[0].fill_(lr_step)
        self._graph.replay()
        self.optimizer.step_count += 1
        self.global_step += 1
        return self._g_loss

    def train_step(self, batch, sync_gradients: bool = True) -> torch.Tensor:
        """One micro-step; returns the (detached) loss."""
        if self._graph is not None and sync_gradients:
            return self._graph_replay(batch)
        cfg = self.cfg
        device_type = self.device.type
        autocast_on = self.weight_dtype != torch.float32 and not self.pure_bf16

        pixel_values = batch["pixel_values"].to(self.device, non_blocking=True)
        if cfg.channels_last and self.device.type == "cuda":
            pixel_values = pixel_values.to(memory_format=torch.channels_last)
        input_ids = batch["input_ids"].to(self.device, non_blocking=True)

        self.ddp.require_backward_grad_sync = sync_gradients

        with torch.autocast(device_type, dtype=self.weight_dtype, enabled=autocast_on):
            with torch.no_grad(), self.prof.phase("vae_encode"):
                latents = self.vae.encode(
                    pixel_values.to(self.weight_dtype)).latent_dist.sample()
                latents = latents * self.vae.config.scaling_factor

                noise = torch.randn_like(latents)
                bsz = latents.shape[0]
                timesteps = torch.randint(
                    0, self.noise_scheduler.num_train_timesteps, (bsz,),
                    device=self.device, dtype=torch.long)
                noisy_latents = self.noise_scheduler.add_noise(latents, noise, timesteps)

            with torch.set_grad_enabled(cfg.train_text_encoder), \
                    self.prof.phase("text_encode"):
                encoder_hidden_states = self.text_encoder(input_ids)[0]
            if cfg.rand_noise_lam > 0:
                encoder_hidden_states = encoder_hidden_states + \
                    cfg.rand_noise_lam * torch.randn_like(encoder_hidden_states)
            if cfg.mixup_noise_lam > 0:
                lam = float(np.random.beta(cfg.mixup_noise_lam, 1))
                index = torch.randperm(encoder_hidden_states.shape[0], device=self.device)
                encoder_hidden_states = lam * encoder_hidden_states + \
                    (1 - lam) * encoder_hidden_states[index]

            with self.prof.phase("unet_fwd"):
                model_pred = self.unet(noisy_latents, timesteps, encoder_hidden_states)

            if self.noise_scheduler.prediction_type == "epsilon":
                target = noise
            elif self.noise_scheduler.prediction_type == "v_prediction":
                target = self.noise_scheduler.get_velocity(latents, noise, timesteps)
            else:
                raise ValueError(self.noise_scheduler.prediction_type)

        loss = F.mse_loss(model_pred.float(), target.float(), reduction="mean")
        # reference parity: accelerator.backward(loss) divides by the
        # accumulation count so accumulated grads are a mean, not a sum
        # (reference diff_train.py:656 via accelerate)
        accum = cfg.gradient_accumulation_steps
        bwd_loss = loss / accum if accum > 1 else loss
        with self.prof.phase("backward"):
            if self.scaler is not None:
                self.scaler.scale(bwd_loss).backward()
            else:
                bwd_loss.backward()

        if sync_gradients:
            with self.prof.phase("optimizer"):
                self.ddp.finalize()
                grads_finite = True
                if self.scaler is not None:
                    # grads were all-reduced BEFORE unscaling, so an overflow
                    # on any rank propagates to every rank -> consistent skip
                    inv = 1.0 / self.scaler.get_scale()
                    self.optimizer.arena_written()
                    self.optimizer.flat_grad.mul_(inv)
                    grads_finite = bool(
                        torch.isfinite(self.optimizer.flat_grad).all())
                if grads_finite:
                    lr_step = get_lr(cfg, self.global_step, self.world)
                    if self.optimizer.hyper is not None:
                        # device-state path: clip fused into the kernels
                        self.optimizer.step_dev(lr=lr_step)
                    else:
                        self.optimizer.clip_and_step(cfg.max_grad_norm,
                                                     lr=lr_step)
                    if self.scaler is not None:
                        # growth bookkeeping is done manually (we never call
                        # scaler.step()/unscale_(), so a bare update() would
                        # assert "No inf checks were recorded"): grow 2x after
                        # growth_interval consecutive finite steps, matching
                        # GradScaler defaults
                        self._finite_streak += 1
                        if self._finite_streak >= 2000:
                            self.scaler.update(self.scaler.get_scale() * 2.0)
                            self._finite_streak = 0
                        else:
                            self.scaler.update(self.scaler.get_scale())
                else:
                    # fp16 overflow: skip the update, back the scale off
                    # (GradScaler semantics; reference utils_ret.py:834-860
                    # relies on torch's internal version of this)
                    self._finite_streak = 0
                    self.scaler.update(self.scaler.get_scale() * 0.5)
                self.optimizer.zero_grad()
            self.global_step += 1
        else:
            # hand the micro-step's gradient to the arena now (scaled, with
            # the fp16 scaler: unscaled once on the sync step): with p.grad
            # left set the next backward would accumulate through one add_
            # per parameter and keep a second copy of the gradient alive
            self.optimizer.gather_grads()
        return loss.detach()

    # ------------------------------------------------------------------
    def fit(self, max_steps: Optional[int] = None, sample_fn=None):
        """Train loop. Failure policy: any exception is
        logged and the process group torn down so peer ranks abort on
        their next collective instead of hanging until the RCCL timeout;
        torchrun then propagates the non-zero exit."""
        try:
            self._fit_inner(max_steps, sample_fn)
        except Exception:
            import traceback
            print(f"rank {self.rank}: training failed\n{traceback.format_exc()}",
                  flush=True)
            if dist_utils.is_dist():
                import torch.distributed as dist
                dist.destroy_process_group()
            raise

    def _fit_inner(self, max_steps: Optional[int] = None, sample_fn=None):
        cfg = self.cfg
        max_steps = max_steps or cfg.max_train_steps
        out_dir = Path(cfg.output_dir)
        if dist_utils.is_main_process():
            out_dir.mkdir(parents=True, exist_ok=True)
            (out_dir / "generations").mkdir(exist_ok=True)
        self.tracker = self.tracker or Tracker(
            cfg.project, name=out_dir.name, config=cfg.to_dict(), out_dir=out_dir)

        self.unet.train()
        if cfg.train_text_encoder:
            self.text_encoder.train()
        accum = cfg.gradient_accumulation_steps
        micro = 0
        done = False
        t0 = time.time()
        for epoch in range(cfg.num_train_epochs):
            if isinstance(getattr(self.dataloader, "sampler", None), DistributedSampler):
                self.dataloader.sampler.set_epoch(epoch)
            for batch in self.dataloader:
                micro += 1
                sync = (micro % accum == 0)
                loss = self.train_step(batch, sync_gradients=sync)
                if sync:
                    lr_now = self.optimizer.lr
                    if self.global_step % cfg.log_every == 0:
                        imgs_s = cfg.train_batch_size * self.world * cfg.log_every \
                            / max(time.time() - t0, 1e-9)
                        self.tracker.log({"loss": loss.item(), "lr": lr_now,
                                          "imgs_per_sec": imgs_s},
                                         step=self.global_step)
                        t0 = time.time()
                    if sample_fn is not None and self.global_step % cfg.save_steps == 0 \
                            and dist_utils.is_main_process():
                        sample_fn(self, out_dir)
                    if self.global_step % cfg.modelsavesteps == 0 \
                            and dist_utils.is_main_process():
                        self.save_checkpoint(out_dir / f"checkpoint_{self.global_step}")
                    if self.global_step >= max_steps:
                        done = True
                        break
            dist_utils.barrier()
            if done:
                break
        if dist_utils.is_main_process():
            self.save_checkpoint(out_dir / "checkpoint")

    # ------------------------------------------------------------------
    def save_checkpoint(self, path):
        """diffusers pipeline layout + state.pt (resume), SURVEY.md §5.4."""
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        self.unet.save_pretrained(path / "unet")
        self.vae.save_pretrained(path / "vae")
        self.text_encoder.save_pretrained(path / "text_encoder")
        self.tokenizer.save_pretrained(path / "tokenizer")
        self.noise_scheduler.save_pretrained(path / "scheduler")
        save_pipeline_index(path)
        state = {
            "global_step": self.global_step,
            "optimizer": self.optimizer.state_dict(),
            "torch_rng": torch.get_rng_state(),
            "numpy_rng": np.random.get_state(),
            "python_rng": random.getstate(),
            "config": self.cfg.to_dict(),
        }
        if torch.cuda.is_available():
            state["cuda_rng"] = torch.cuda.get_rng_state_all()
        torch.save(state, path / "state.pt")

    def load_checkpoint(self, path):
        path = Path(path)
        from ..models.model_io import load_module
        load_module(self.unet, path / "unet")
        load_module(self.vae, path / "vae")
        load_module(self.text_encoder, path / "text_encoder")
        state_f = path / "state.pt"
        if state_f.exists():
            st = torch.load(state_f, map_location="cpu", weights_only=False)
            self.global_step = st["global_step"]
            self.optimizer.load_state_dict(st["optimizer"])
            # restore RNG streams so resumed training is bit-faithful
            if "torch_rng" in st:
                torch.set_rng_state(st["torch_rng"].cpu().to(torch.uint8))
            if "numpy_rng" in st:
                np.random.set_state(st["numpy_rng"])
            if "python_rng" in st:
                random.setstate(st["python_rng"])
            if "cuda_rng" in st and torch.cuda.is_available():
                try:
                    torch.cuda.set_rng_state_all(
                        [t.cpu().to(torch.uint8) for t in st["cuda_rng"]])
                except Exception as e:
                    print(f"cuda rng restore skipped: {e}")
