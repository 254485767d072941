"""optim.ClipAdamW on CPU parameters (the torch-op path) and its state_dict
against torch.optim.AdamW: every parameter's step is its own
tensor in the state_dict, so an AdamW loading it advances each once per step
(a shared step tensor was advanced once per parameter), and a parameter
without a gradient keeps its step, as in torch."""
import torch


def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(n)) for n in (3, 5, 2)]


def test_state_dict_steps_are_per_parameter_for_torch_adamw():
    from mcaq_yolo_amd.optim import ClipAdamW
    ps = _params()
    o = ClipAdamW(ps, lr=1e-2, weight_decay=0.05, max_norm=1.0)
    for p in ps:
        p.grad = torch.ones_like(p)
    o.step()
    t = torch.optim.AdamW(ps, lr=1e-2, weight_decay=0.05)
    t.load_state_dict(o.state_dict())
    t.step()
    assert [float(t.state[p]["step"]) for p in ps] == [2.0, 2.0, 2.0]
    # ClipAdamW's own counters were not touched by torch's step
    assert [float(o.state[p]["step"]) for p in ps] == [1.0, 1.0, 1.0]


def test_matches_torch_adamw_with_unused_parameter():
    from mcaq_yolo_amd.optim import ClipAdamW
    ps, qs = _params(), _params()
    o0 = torch.optim.AdamW(ps, lr=1e-2, weight_decay=0.05, foreach=False)
    o1 = ClipAdamW(qs, lr=1e-2, weight_decay=0.05)
    g = torch.Generator().manual_seed(1)
    for it in range(4):
        gs = [torch.randn(p.shape, generator=g) for p in ps]
        for k, (p, q, gg) in enumerate(zip(ps, qs, gs)):
            use = not (k == 1 and it in (1, 2))         # parameter 1 unused on steps 1 and 2
            p.grad = gg.clone() if use else None
            q.grad = gg.clone() if use else None
        o0.step()
        o1.step()
    for p, q in zip(ps, qs):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)
        assert float(o0.state[p]["step"]) == float(o1.state[q]["step"])
    assert float(o1.state[qs[1]]["step"]) == 2.0


def test_load_state_dict_roundtrip():
    from mcaq_yolo_amd.optim import ClipAdamW
    ps = _params()
    o = ClipAdamW(ps, lr=1e-2)
    for p in ps:
        p.grad = torch.ones_like(p)
    o.step()
    o.step()
    o2 = ClipAdamW(ps, lr=1e-2)
    o2.load_state_dict(o.state_dict())
    for p in ps:
        assert torch.equal(o2.state[p]["exp_avg"], o.state[p]["exp_avg"])
        assert float(o2.state[p]["step"]) == 2.0


def test_add_param_group_after_a_step_matches_torch_adamw():
    """A group added with add_param_group after the first step (its own lr):
    the new parameter starts from zero moments at step 0, the old ones keep
    their moments and steps - torch.optim.AdamW doing the same."""
    from mcaq_yolo_amd.optim import ClipAdamW
    ps, qs = _params(), _params()
    o0 = torch.optim.AdamW(ps[:2], lr=1e-2, weight_decay=0.05, foreach=False)
    o1 = ClipAdamW(qs[:2], lr=1e-2, weight_decay=0.05)
    g = torch.Generator().manual_seed(2)
    for it in range(4):
        if it == 2:
            o0.add_param_group(dict(params=[ps[2]], lr=3e-3))
            o1.add_param_group(dict(params=[qs[2]], lr=3e-3))
        live = 2 if it < 2 else 3
        for p, q in zip(ps[:live], qs[:live]):
            gg = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gg.clone(), gg.clone()
        o0.step()
        o1.step()
        if it == 1:
            kept = [o1.state[q]["exp_avg"].clone() for q in qs[:2]]
    for p, q in zip(ps, qs):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)
        assert torch.allclose(o0.state[p]["exp_avg_sq"], o1.state[q]["exp_avg_sq"], rtol=1e-6, atol=1e-12)
        assert float(o0.state[p]["step"]) == float(o1.state[q]["step"])
    assert [float(o1.state[q]["step"]) for q in qs] == [4.0, 4.0, 2.0]
    assert all(not torch.equal(k, o1.state[q]["exp_avg"]) for k, q in zip(kept, qs[:2]))
    assert len(o1.state_dict()["state"]) == 3


def test_empty_parameter_is_left_out_of_the_step():
    """A parameter with numel() == 0 and a gradient is no segment of the step
    (torch tolerates it too): the others step as without it, with clipping."""
    from mcaq_yolo_amd.optim import ClipAdamW
    ps, qs = _params(), _params()
    e = torch.nn.Parameter(torch.zeros(0, 4))
    o0 = ClipAdamW(ps, lr=1e-2, weight_decay=0.05, max_norm=0.5)
    o1 = ClipAdamW([qs[0], e] + qs[1:], lr=1e-2, weight_decay=0.05, max_norm=0.5)
    g = torch.Generator().manual_seed(3)
    for it in range(2):
        for p, q in zip(ps, qs):
            gg = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gg.clone(), gg.clone()
        e.grad = torch.zeros_like(e)
        o0.step()
        o1.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
    assert torch.equal(o0.last_total_norm, o1.last_total_norm)
    assert e.numel() == 0 and len(o1.state_dict()["state"]) == 4
