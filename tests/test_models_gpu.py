"""GPU end-to-end tests for the non-GPT model families (MoE, Wide-ResNet):
the HIP kernel path must run them (no eager fallback)."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_gpt_moe_gpu_trains():
    from tepdist_amd.models.configs import MOE_CONFIGS
    from tepdist_amd.models.moe import GPTMoE
    from tepdist_amd.train import AdamW, Trainer
    cfg = MOE_CONFIGS["gpt-moe-test"]
    torch.manual_seed(0)
    model = GPTMoE(cfg, dtype=torch.bfloat16).cuda()
    opt = AdamW(model.parameters(), lr=1e-3)
    trainer = Trainer(model, opt)
    ids = torch.randint(0, cfg.vocab_size, (4, 33),
                        generator=torch.Generator().manual_seed(1)).cuda()
    losses = [trainer.train_step(lambda i: (ids[:, :-1], ids[:, 1:]))
              for _ in range(8)]
    assert losses[-1] < losses[0], losses


def test_wide_resnet_gpu_trains():
    from tepdist_amd.models.configs import WIDE_RESNET_CONFIGS
    from tepdist_amd.models.wide_resnet import WideResNet
    from tepdist_amd.train import AdamW, Trainer
    cfg = WIDE_RESNET_CONFIGS["wrn-test"]
    torch.manual_seed(0)
    model = WideResNet(cfg, dtype=torch.bfloat16).cuda()
    opt = AdamW(model.parameters(), lr=5e-4)
    trainer = Trainer(model, opt)
    x = torch.randn(8, 3, 32, 32).bfloat16().cuda()
    y = torch.randint(0, cfg.num_classes, (8,)).cuda()
    losses = [trainer.train_step(lambda i: (x, y)) for _ in range(8)]
    assert losses[-1] < losses[0] * 1.05, losses


def test_rpc_service_gpu_step(tmp_path):
    """Server-side IR interpreter executes on the GPU through the kernels."""
    from tepdist_amd.ir import gpt2_ir
    from tepdist_amd.models.configs import GPT2_CONFIGS
    from tepdist_amd.rpc.service import TepdistService
    cfg = GPT2_CONFIGS["gpt2-test"]
    svc = TepdistService(ckpt_dir=str(tmp_path / "ckpt"))
    assert svc.device.startswith("cuda")
    g = gpt2_ir(cfg, batch=4, seq=16)
    r = svc.build_execution_plan({"graph": g.to_json(), "num_devices": 1})
    ids = torch.randint(0, cfg.vocab_size, (4, 17),
                        generator=torch.Generator().manual_seed(2))
    feeds = {"input_ids": ids[:, :-1].reshape(-1),
             "labels": ids[:, 1:].reshape(-1)}
    losses = []
    for _ in range(6):
        out = svc.execute_plan({"handle": r["handle"], "inputs": feeds})
        losses.append(float(list(out["outputs"].values())[0]))
    assert losses[-1] < losses[0], losses


def test_llama_ops_gpu_match_reference():
    from tepdist_amd.ops import hip, reference as ref

    torch.manual_seed(0)
    x = torch.randn(64, 2048).bfloat16().cuda()
    g = torch.randn(2048).bfloat16().cuda()
    y, rstd = hip.rmsnorm_fwd(x, g)
    yr, rr = ref.rmsnorm_fwd(x.float().cpu(), g.float().cpu())
    assert torch.allclose(y.float().cpu(), yr, atol=3e-2)
    dy = torch.randn_like(x)
    dx, dg = hip.rmsnorm_bwd(dy, x, g, rstd)
    dxr, dgr = ref.rmsnorm_bwd(dy.float().cpu(), x.float().cpu(),
                               g.float().cpu(), rr)
    assert torch.allclose(dx.float().cpu(), dxr, atol=5e-2)
    assert torch.allclose(dg.float().cpu(), dgr.float(), atol=1.0,
                          rtol=3e-2)

    q = torch.randn(256, 16, 128).bfloat16().cuda()
    yq = hip.rope_fwd(q, seq_len=64)
    yqr = ref.rope_fwd(q.float().cpu(), seq_len=64)
    assert torch.allclose(yq.float().cpu(), yqr, atol=3e-2)
    back = hip.rope_bwd(yq, seq_len=64)
    assert torch.allclose(back.float().cpu(), q.float().cpu(), atol=3e-2)

    a = torch.randn(4096).bfloat16().cuda()
    b = torch.randn(4096).bfloat16().cuda()
    ys = hip.swiglu_fwd(a, b)
    ysr = ref.swiglu_fwd(a.float().cpu(), b.float().cpu())
    assert torch.allclose(ys.float().cpu(), ysr, atol=3e-2)
    da, db = hip.swiglu_bwd(torch.ones_like(ys), a, b)
    dar, dbr = ref.swiglu_bwd(torch.ones(4096), a.float().cpu(),
                              b.float().cpu())
    assert torch.allclose(da.float().cpu(), dar, atol=3e-2)
    assert torch.allclose(db.float().cpu(), dbr, atol=3e-2)


def test_llama_gpu_trains():
    from tepdist_amd.models.llama import LLAMA_CONFIGS, Llama
    from tepdist_amd.train.optim import AdamW

    torch.manual_seed(0)
    cfg = LLAMA_CONFIGS["llama-test"]
    model = Llama(cfg, dtype=torch.bfloat16).cuda()
    opt = AdamW(model.parameters(), lr=3e-3)
    ids = torch.randint(0, cfg.vocab_size, (2, 65), device="cuda")
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = model(ids[:, :-1], labels=ids[:, 1:])
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 0.5, losses


def test_generation_engine_gpu():
    from tepdist_amd.inference import Generator
    from tepdist_amd.models import GPT2, GPT2_CONFIGS

    torch.manual_seed(0)
    cfg = GPT2_CONFIGS["gpt2-test"]
    model = GPT2(cfg, dtype=torch.bfloat16).cuda().eval()
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device="cuda")
    out = Generator(model).generate(ids, max_new_tokens=8)
    assert out.shape == (2, 20)
    assert (out[:, :12] == ids).all()
    assert (out < cfg.vocab_size).all()


@pytest.mark.gpu
def test_planned_graph_gpu_step():
    """The flagship bench path in miniature: AutoParallel plan ->
    PlannedModule (multi-round transform + interpreter over the CDNA4
    kernels) -> Trainer step with the plan's optimizer on cuda:0."""
    from tepdist_amd.ir.capture import gpt2_ir
    from tepdist_amd.models.configs import GPT2_CONFIGS
    from tepdist_amd.planner.auto_parallel import AutoParallel
    from tepdist_amd.runtime.planned import PlannedModule
    from tepdist_amd.train import Trainer
    cfg = GPT2_CONFIGS["gpt2-test"]
    g = gpt2_ir(cfg, batch=4, seq=32)
    plan = AutoParallel(g, 1).run()
    m = PlannedModule(g, plan, device="cuda:0", dtype=torch.bfloat16)
    opt = m.make_optimizer(lr=1e-3)
    tr = Trainer(m, opt, grad_accum_steps=1)
    torch.manual_seed(0)
    ids = torch.randint(0, cfg.vocab_size, (4, 33), device="cuda")
    losses = [tr.train_step(lambda i: (ids[:, :-1], ids[:, 1:]))
              for _ in range(4)]
    assert losses[-1] < losses[0], losses
    assert tr._graph is not None, "planned path should capture a hipGraph"


@pytest.mark.gpu
def test_moe_ir_graph_gpu():
    """The MoE planner IR executes on GPU through the interpreter
    (moe_dispatch/combine + batched expert matmuls on the kernel set)."""
    from tepdist_amd.ir.capture import moe_ir
    from tepdist_amd.ir.interpreter import GraphInterpreter
    from tepdist_amd.models.configs import MOE_CONFIGS
    from tepdist_amd.runtime.initializers import default_init_spec, \
        init_shard
    cfg = MOE_CONFIGS["gpt-moe-test"]
    g = moe_ir(cfg, batch=2, seq=16, capacity_factor=4.0)
    vars_ = {}
    for name, nid in g.params.items():
        sh = g.nodes[nid].shape
        t = init_shard(name, tuple(sh), default_init_spec(name, sh),
                       dtype=torch.bfloat16)
        vars_[name] = t.cuda().requires_grad_()
    gen = torch.Generator().manual_seed(3)
    feeds = {"input_ids": torch.randint(0, cfg.vocab_size, (32,),
                                        generator=gen).cuda(),
             "labels": torch.randint(0, cfg.vocab_size, (32,),
                                     generator=gen).cuda()}
    interp = GraphInterpreter(g, "cuda:0", dtype=torch.bfloat16)
    loss = list(interp.run(feeds, vars_).values())[0]
    loss.backward()
    assert torch.isfinite(loss)
    assert vars_["h0.moe_w1"].grad is not None
    assert torch.isfinite(vars_["h0.moe_w1"].grad).all()


@pytest.mark.gpu
def test_ring_attention_flash_gpu():
    """Ring attention's per-block flash path (world 1 degenerates to one
    diagonal block): bf16 flash kernels vs the fp32 composed reference."""
    from tepdist_amd.parallel.ring_attention import ring_attention
    torch.manual_seed(0)
    B, H, S, D = 2, 4, 256, 64
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    k = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    v = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    out = ring_attention(q, k, v, causal=True)
    out.float().sum().backward()
    q2, k2, v2 = (t.detach().float().clone().requires_grad_()
                  for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(
        q2, k2, v2, is_causal=True)
    ref.sum().backward()
    torch.testing.assert_close(out.float(), ref, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(q.grad.float(), q2.grad, rtol=5e-2,
                               atol=5e-2)
    torch.testing.assert_close(k.grad.float(), k2.grad, rtol=5e-2,
                               atol=5e-2)
    torch.testing.assert_close(v.grad.float(), v2.grad, rtol=5e-2,
                               atol=5e-2)
