"""The reference's precision policy as a mode, the parts that need no GPU: the two CLIs' new arguments, the host-side plan
of the in-step merge for f32 sources (``lora_amd_mstep_site.src_f32``), and ``StepConfig.reference_add_noise``."""
import ctypes as C
import inspect
import os
import sys
import types

import pytest
import torch

from lora_amd import _C, ops
from lora_amd import trainer as T
from lora_amd.standin import DDPMScheduler
from oracle import torch_ref as TR
from tests.helpers import REPO

sys.path.insert(0, os.path.join(REPO, "training_scripts"))
import train_lora_dreambooth as cli  # noqa: E402

BASE = ["--pretrained_model_name_or_path", "standin", "--standin", "tiny", "--instance_data_dir", "synthetic:4",
        "--instance_prompt", "a photo of sks dog", "--resolution", "64", "--train_batch_size", "2", "--learning_rate",
        "1e-3", "--lr_scheduler", "constant", "--lr_warmup_steps", "0", "--device", "cpu", "--seed", "3"]


def test_both_clis_carry_the_new_arguments_with_todays_defaults():
    args = cli.parse_args(BASE)
    assert args.frozen_dtype == "compute" and args.reference_add_noise is False
    args = cli.parse_args(BASE + ["--frozen_dtype", "fp32", "--reference_add_noise"])
    assert args.frozen_dtype == "fp32" and args.reference_add_noise is True
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + ["--frozen_dtype", "bf16"])
    from lora_amd import cli_lora_pti as pti

    ps = list(inspect.signature(pti.train).parameters.values())
    names = [p.name for p in ps]
    assert names.index("frozen_dtype") >= 55 and names.index("reference_add_noise") >= 55
    assert ps[names.index("frozen_dtype")].default == "compute" and ps[names.index("reference_add_noise")].default is False
    assert "MASTER_MERGE" in ops.apply_ab_overrides("MASTER_MERGE=0", {}) and ops.MASTER_MERGE is True
    assert T.StepConfig().reference_add_noise is False


def _table(src_f32s, shapes=((320, 320, 4), (2560, 328, 16))):
    sites = (_C.MstepSite * len(shapes))()
    for s, (N, K, r), f in zip(sites, shapes, src_f32s):
        s.N, s.K, s.r = N, K, r
        s.w = s.up = s.down = s.out = 4096
        s.ld_out = K
        s.src_f32 = f
    return sites


def test_plan_of_an_f32_source_table_has_the_same_tiles_and_sets_the_source_bit():
    """The field that was ``reserved`` keeps its offset and the struct its size; a table of f32 sources plans to the same
    tile count and geometry bits as the 16-bit table and carries a bit at or above bit 48."""
    assert _C.MstepSite.src_f32.offset == 92 and C.sizeof(_C.MstepSite) == 104 and _C.MstepSite.tile_begin.offset == 96
    lib = _C.require()
    assert lib.lora_amd_abi_version() == 8
    for tile in range(4):
        vals = {}
        for f in (0, 1):
            sites, val = _table([f, f]), C.c_int64(0)
            _C.merge_step_set_tuning(tile, -1)
            try:
                assert lib.lora_amd_merge_step_plan(sites, 2, _C.BF16, C.byref(val)) == 0
            finally:
                _C.merge_step_set_tuning(2, -1)
            vals[f] = (val.value, sites[1].tile_begin, sites[1].tiles_k)
        v0, v1 = vals[0][0], vals[1][0]
        assert v0 >> 40 == tile                                   # a 16-bit table's value is what it was
        assert v1 != v0 and v1 >> 48 != 0 and v0 >> 48 == 0       # the source bit
        assert v1 & ((1 << 40) - 1) == v0 & ((1 << 40) - 1)       # tile count
        assert (v1 >> 40) & 0xFF == tile                          # geometry
        assert vals[0][1:] == vals[1][1:]


def test_plan_refuses_mixed_tables_and_f32_outputs():
    lib = _C.require()
    val = C.c_int64(0)
    assert lib.lora_amd_merge_step_plan(_table([0, 1]), 2, _C.BF16, C.byref(val)) != 0
    msg = lib.lora_amd_last_error()
    assert b"site 1" in msg and b"src_f32" in msg, msg
    assert lib.lora_amd_merge_step_plan(_table([1, 0]), 2, _C.F16, C.byref(val)) != 0
    assert b"site 1" in lib.lora_amd_last_error()
    assert lib.lora_amd_merge_step_plan(_table([2, 2]), 2, _C.BF16, C.byref(val)) != 0
    for f in (0, 1):   # w_dtype is the OUTPUT dtype: f32 stays refused
        assert lib.lora_amd_merge_step_plan(_table([f, f]), 2, _C.F32, C.byref(val)) != 0
    # a zero-initialised table (src_f32 = 0): the value of the plan as it always was — 128 x 128 tiles, no high bits
    assert lib.lora_amd_merge_step_plan(_table([0, 0]), 2, _C.BF16, C.byref(val)) == 0
    want = sum(-(-N // 128) * -(-K // 128) for N, K in ((320, 320), (2560, 328)))
    assert val.value == want | (2 << 40)


class _Recorder(torch.nn.Module):
    """A UNet-shaped toy: remembers its input, returns it times one trainable scalar."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.ones(()))
        self.seen = None

    def forward(self, x, t, ehs):
        self.seen = x.detach().clone()
        return types.SimpleNamespace(sample=x.float() * self.p)


def test_reference_add_noise_is_the_oracles_formula_in_the_latents_dtype():
    """``StepConfig(reference_add_noise=True)``: the UNet's input is oracle.torch_ref.dreambooth_step's add_noise evaluated
    in bf16, bit for bit — a t = 0 sample comes through un-noised (bf16(alpha_bar_0) = 1); the default stays the f32-formed
    value rounded once."""
    g = torch.Generator().manual_seed(5)
    lat = (torch.randn(4, 4, 8, 8, generator=g) * 0.18215).to(torch.bfloat16)
    noise = torch.randn(4, 4, 8, 8, generator=g).to(torch.bfloat16)
    ts = torch.tensor([0, 3, 500, 999])
    ehs = torch.zeros(4, 77, 8)
    sched = DDPMScheduler()
    seen = {}

    def oracle_unet(x, tt, c):
        seen["oracle"] = x.detach().clone()
        return x.float() * p

    p = torch.nn.Parameter(torch.ones(()))
    TR.dreambooth_step(oracle_unet, [p], torch.optim.SGD([p], lr=0.0), lat, noise, ts, ehs, sched.alphas_cumprod)
    assert seen["oracle"].dtype == torch.bfloat16

    unet = _Recorder()
    T.forward_backward(unet, sched, lat, ehs, T.StepConfig(reference_add_noise=True), noise=noise, timesteps=ts)
    assert unet.seen.dtype == torch.bfloat16 and torch.equal(unet.seen, seen["oracle"])
    assert float(sched.alphas_cumprod[0].to(torch.bfloat16)) == 1.0
    assert torch.equal(unet.seen[0], lat[0])          # t = 0: no noise at all under the reference's arithmetic
    assert unet.p.grad is not None

    T.forward_backward(unet, sched, lat, ehs, T.StepConfig(), noise=noise, timesteps=ts)
    a = sched.alphas_cumprod[ts].view(-1, 1, 1, 1)
    want = (a.sqrt() * lat.float() + (1 - a).sqrt() * noise.float()).to(torch.bfloat16)
    assert torch.equal(unet.seen, want)
    assert not torch.equal(unet.seen[0], lat[0])      # ... while the default keeps the noise of a t = 0 sample
    assert not torch.equal(unet.seen, seen["oracle"])

    # f32 latents: both settings are the same arithmetic
    outs = []
    for flag in (False, True):
        T.forward_backward(unet, sched, lat.float(), ehs, T.StepConfig(reference_add_noise=flag), noise=noise.float(),
                           timesteps=ts)
        outs.append(unet.seen)
    assert torch.equal(outs[0], outs[1])


def test_cli_with_fp32_frozen_dtype_runs_on_the_cpu_and_writes_the_same_files(tmp_path):
    """On the CPU (and with --mixed_precision no) the mode is a no-op: same files, same trained values."""
    outs = {}
    for name, extra in (("plain", []), ("fp32", ["--frozen_dtype", "fp32", "--reference_add_noise"])):
        out = str(tmp_path / name)
        args = cli.parse_args(BASE + ["--output_dir", out, "--max_train_steps", "2", "--train_text_encoder",
                                      "--mixed_precision", "bf16", "--lora_rank", "2"] + extra)
        assert cli.main(args) == 2
        outs[name] = out
    assert set(os.listdir(outs["plain"])) == set(os.listdir(outs["fp32"]))
    assert {"lora_weight.pt", "lora_weight.text_encoder.pt", "lora_weight.safetensors", "logs"} <= set(os.listdir(outs["fp32"]))
    a, b = (torch.load(os.path.join(outs[k], "lora_weight.pt")) for k in ("plain", "fp32"))
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert float(b[0].float().abs().max()) > 0
