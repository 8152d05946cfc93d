"""The reference's command-line workflow end to end on the MI355X with tiny synthetic data:
train_clean_classifier -> train_generator (fresh, then --continue_training) -> train_victim -> eval,
checking the checkpoint layout (paths and keys of reference train_generator.py:441-457, 497-499)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, *args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--synthetic_size", "256", "--bs", "64",
           "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1"] + list(args)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_reference_workflow_on_synthetic_data(tmp_path):
    cwd = str(tmp_path)
    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", "--n_iters", "1", cwd=cwd)
    clean = os.path.join(cwd, "ckpt", "classifier_clean", "cifar10", "cifar10_classifier_clean.pth.tar")
    sd = torch.load(clean, map_location="cpu", weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "best_clean_acc", "epoch_current"}
    assert len(sd["netC"]) == 102 and sd["netC"]["conv1.weight"].shape == (64, 3, 3, 3)

    out = run("train_generator.py", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "classifier_clean",
              "--n_iters", "1", cwd=cwd)
    assert "Clean Acc:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "train_generator_clean", "cifar10", "cifar10_train_generator_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model",
                       "best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
                       "best_clean_model_bd_asr", "epoch_current"}
    assert len(sd["netG"]) == 32 and len(sd["netC"]) == 102
    imgs = os.path.join(cwd, "ckpt", "train_generator_clean", "cifar10", "log_dir", "images")     # :310-315, epoch 0
    assert (os.path.isdir(imgs) and any(f.endswith(".ppm") for f in os.listdir(imgs))) or "tensorboard" in sys.modules
    mom = sd["optimizerG"]["state"]
    assert len(mom) == 32 and all("momentum_buffer" in v for v in mom.values())
    assert all(torch.isfinite(v).all() for v in sd["netG"].values())
    # a torch module of the reference layout can consume the checkpoint as is
    ref_like = torch.nn.Conv2d(3, 64, 3, 2, 1)
    ref_like.load_state_dict({"weight": sd["netG"]["conv0_0.weight"], "bias": sd["netG"]["conv0_0.bias"]})

    out = run("train_generator.py", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "classifier_clean",
              "--n_iters", "2", "--continue_training", cwd=cwd)
    assert "Continue training!!" in out

    run("train_victim.py", "--saving_prefix", "train_victim", "--load_checkpoint", "train_generator_clean",
        "--n_iters", "1", cwd=cwd)
    vic = os.path.join(cwd, "ckpt", "train_victim", "cifar10", "cifar10_train_victim.pth.tar")
    assert set(torch.load(vic, map_location="cpu", weights_only=True)) == {
        "netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "epoch_current"}

    out = run("eval.py", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "train_victim",
              "--load_checkpoint", "train_generator_clean", cwd=cwd)
    assert "Bd ASR:" in out


def test_celeba_workflow_on_synthetic_data(tmp_path):
    """The same three scripts with --dataset celeba (64 x 64, 8 classes, ResNet18 surrogate / clean model,
    train_generator.py:93-96): checkpoints carry the reference's ResNet18 state-dict layout (122 entries)."""
    cwd = str(tmp_path)
    run("train_clean_classifier.py", "--dataset", "celeba", "--saving_prefix", "classifier_clean", "--n_iters", "1", cwd=cwd)
    clean = os.path.join(cwd, "ckpt", "classifier_clean", "celeba", "celeba_classifier_clean.pth.tar")
    sd = torch.load(clean, map_location="cpu", weights_only=True)
    assert len(sd["netC"]) == 122 and sd["netC"]["linear.weight"].shape == (8, 2048)
    out = run("train_generator.py", "--dataset", "celeba", "--saving_prefix", "train_generator",
              "--load_checkpoint_clean", "classifier_clean", "--n_iters", "1", cwd=cwd)
    assert "Clean Acc:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "train_generator_clean", "celeba", "celeba_train_generator_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert len(sd["netC"]) == 122 and len(sd["netG"]) == 32
    assert all(torch.isfinite(v).all() for v in sd["netG"].values())
    assert all(torch.isfinite(v.float()).all() for v in sd["netC"].values())
    out = run("eval.py", "--dataset", "celeba", "--saving_prefix", "train_generator", "--load_checkpoint_clean",
              "classifier_clean", "--load_checkpoint", "train_generator_clean", cwd=cwd)
    assert "Bd ASR:" in out


def test_wanet_workflow_on_synthetic_data(tmp_path):
    """train_generator_wanet.py (reference :455-603): fresh run, checkpoint with the GridGenerator's 20-entry state
    dict under the reference's keys, --continue_training, and eval of the warped test images."""
    cwd = str(tmp_path)
    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", "--n_iters", "1", cwd=cwd)
    out = run("train_generator_wanet.py", "--saving_prefix", "train_generator_wanet", "--load_checkpoint_clean", "classifier_clean",
              "--n_iters", "1", "--s", "2", "--grid_rescale", "0.15", cwd=cwd)
    assert "Clean Acc:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "train_generator_wanet_clean", "cifar10", "cifar10_train_generator_wanet_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model",
                       "best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
                       "best_clean_model_bd_asr", "epoch_current"}
    assert len(sd["netG"]) == 20 and sd["netG"]["fc2.weight"].shape == (8, 64) and sd["netG"]["fc1.weight"].shape == (64, 512)
    assert all(torch.isfinite(v).all() for v in sd["netG"].values())
    assert len(sd["optimizerG"]["state"]) == 20
    out = run("train_generator_wanet.py", "--saving_prefix", "train_generator_wanet", "--load_checkpoint_clean", "classifier_clean",
              "--n_iters", "2", "--continue_training", cwd=cwd)
    assert "Continue training!!" in out
    # the rest of the WaNet pipeline (reference train_victim_wanet.py): victim on warped poisoned images, checkpoint
    # under <prefix>_clean/ with the extra grid_rescale key (:199, :241-243), image grid logged every epoch (:136)
    out = run("train_victim_wanet.py", "--saving_prefix", "train_victim_wanet", "--load_checkpoint", "train_generator_wanet_clean",
              "--n_iters", "1", "--grid_rescale", "0.15", cwd=cwd)
    assert "Bd Acc:" in out
    vic = os.path.join(cwd, "ckpt", "train_victim_wanet_clean", "cifar10", "cifar10_train_victim_wanet_clean.pth.tar")
    sdv = torch.load(vic, map_location="cpu", weights_only=True)
    assert set(sdv) == {"netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "epoch_current", "grid_rescale"}
    assert len(sdv["netG"]) == 20 and len(sdv["netC"]) == 102
    imgs = os.path.join(cwd, "ckpt", "train_victim_wanet_clean", "cifar10", "log_dir", "images")
    assert os.path.isdir(imgs) and any(f.endswith(".ppm") for f in os.listdir(imgs)) or "tensorboard" in sys.modules
    # train_victim.py refuses the WaNet generator by name; eval.py accepts it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_victim.py"), "--synthetic", "--synthetic_size", "256", "--bs", "64",
                        "--checkpoints", os.path.join(cwd, "ckpt"), "--saving_prefix", "train_victim_refused", "--load_checkpoint",
                        "train_generator_wanet_clean", "--n_iters", "1"],
                       cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "train_victim_wanet.py" in (r.stdout + r.stderr)
    out = run("eval.py", "--saving_prefix", "train_generator_wanet", "--load_checkpoint_clean", "train_victim_wanet_clean",
              "--load_checkpoint", "train_generator_wanet_clean", cwd=cwd)
    assert "Bd ASR:" in out


def test_wanet_celeba_workflow_on_synthetic_data(tmp_path):
    """train_generator_wanet.py --dataset celeba (reference :63-66: 64 x 64, 8 classes, ResNet18 surrogate / clean model,
    GridGenerator warp at 64 x 64)."""
    cwd = str(tmp_path)
    common = ["--dataset", "celeba", "--n_iters", "1"]
    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", *common, cwd=cwd)
    out = run("train_generator_wanet.py", "--saving_prefix", "train_generator_wanet", "--load_checkpoint_clean", "classifier_clean",
              *common, cwd=cwd)
    assert "Clean Acc:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "train_generator_wanet_clean", "celeba", "celeba_train_generator_wanet_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert sd["netC"]["linear.weight"].shape == (8, 2048) and len(sd["netG"]) == 20
    assert all(torch.isfinite(v.float()).all() for v in sd["netC"].values())
    assert all(torch.isfinite(v).all() for v in sd["netG"].values())


def test_wanet_imagenet10_workflow_on_synthetic_data(tmp_path):
    """BASELINE config 5: --dataset imagenet10 (224 x 224, 10 classes, ResNet18(input_size=224), bs forced to 32 as
    reference train_generator_wanet.py:471-476).  The reference itself raises KeyError here."""
    cwd = str(tmp_path)
    common = ["--dataset", "imagenet10", "--synthetic_size", "64", "--n_iters", "1"]
    out = run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", *common, cwd=cwd)
    out = run("train_generator_wanet.py", "--saving_prefix", "train_generator_wanet", "--load_checkpoint_clean", "classifier_clean",
              *common, cwd=cwd)
    assert "Clean Acc:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "train_generator_wanet_clean", "imagenet10", "imagenet10_train_generator_wanet_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert sd["netC"]["linear.weight"].shape == (10, 512 * 49) and len(sd["netG"]) == 20
    assert all(torch.isfinite(v.float()).all() for v in sd["netC"].values())


def _two_rank_rehearsal(worker, out_dir):
    """Start `worker` as two fresh rank processes on this box's one GPU (exchange over gloo) and return both ranks'
    result JSON.  One child, no retry; a non-zero exit fails with the tail of its output."""
    import json
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", worker), str(out_dir)]
    env = dict(os.environ, PYTHONPATH=ROOT, COMBAT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return [json.load(open(out_dir / ("rank%d.json" % rank))) for rank in (0, 1)]


def _assert_reduced_generator_gradient(res, tag):
    """tests/dp_rehearsal.py::gen_grad_check: at lr_c = 0.0 netC stays what it was (the precondition that makes a
    single-process run a reference for Phase G), the reduced generator gradient is the sum of the two ranks'
    single-process gradients (the bound of the same identity on netC: fp32 atomics in some weight-gradient launches
    reorder sums) and not this rank's own (100 x the bound: the exchange added the other shard, and the shards
    differ), and the optimiser applied their mean.  The repeat noise of the reference is recorded beside it.

    Measured on the MI355X (rel. L2; error of the sum / repeat noise of a single-process run): alternated 5.5e-8 /
    4.7e-8 .. 5.5e-8, input-aware 4.2e-8 / 3.3e-8 .. 3.9e-8, imperceptible 3.8e-8 / 3.2e-8 .. 3.5e-8, WaNet head 0 / 0
    (its backward has no atomics); in the library's deterministic mode all of them are exactly 0.  Against this rank's
    own gradient 0.61 .. 1.65, between the two singles 1.2 .. 1.4.  Update against the mean 4e-11 .. 2.3e-9; the same
    tensors against the SUM of the singles 9e-6 (input-aware, lr_g 1e-3) .. 2e-4."""
    print(tag, {k: v for k, v in res.items() if k.startswith(tag + "_")})
    assert res[tag + "_netC_unchanged"] is True, (tag, res)
    assert res[tag + "_noise"] >= 0.0, (tag, res)
    assert res[tag + "_gradG_sum_vs_singles"] < 1e-5, (tag, res)
    assert res[tag + "_gradG_vs_own"] > 1e-3 and res[tag + "_gradG_singles_differ"] > 1e-3, (tag, res)
    assert res[tag + "_paramG_update_vs_mean_grad"] < 1e-6, (tag, res)


def test_data_parallel_step_two_ranks_one_gpu(tmp_path):
    """SURVEY 8(e) without an 8-GPU node: two fresh rank processes share this box's GPU and exchange over gloo
    (tests/dp_rehearsal.py).  After step 1 the all-reduced netC gradient is the sum of the two single-rank
    gradients (rel <= 1e-5: fp32 atomics in some weight-gradient launches reorder sums) and the optimiser
    applied their MEAN; netG's reduced gradient is the same bits on both ranks; after 2 steps parameters and
    momentum of both trained networks are bit-identical replicas.  The same for ClassifierStep (train_victim.py behind
    a UNet, train_victim_wanet.py behind a GridGenerator, train_clean_classifier.py) and WanetStep, whose all-reduces
    take other routes (plan marks of the victim's backward; the grid head's gradient range).  For AlternatedStep and
    WanetStep the reduced GENERATOR gradient is also checked by value (_assert_reduced_generator_gradient).
    10.7 s on the MI355X."""
    for res in _two_rank_rehearsal("dp_rehearsal.py", tmp_path):
        assert res["gradC_sum_vs_singles"] < 1e-5, res
        assert res["paramC_update_vs_mean_grad"] < 1e-6, res
        assert res["gradG_identical_across_ranks"] and res["replicas_bit_identical_after_2_steps"] and res["finite"], res
        # ClassifierStep (victim behind a UNet / a GridGenerator, clean classifier) and WanetStep: same properties
        for tag in ("clf_unet", "clf_grid", "clf_clean"):
            assert res[tag + "_grad_sum_vs_singles"] < 1e-5, (tag, res)
            assert res[tag + "_grad_identical_across_ranks"] and res[tag + "_replicas_bit_identical_after_2_steps"], (tag, res)
        assert res["wanet_head_grad_identical_across_ranks"] and res["wanet_head_grad_nonzero"], res
        assert res["wanet_grad_outside_head_range_is_zero"] and res["wanet_gradC_identical_across_ranks"], res
        assert res["wanet_replicas_bit_identical_after_2_steps"], res
        # the reduced GENERATOR gradient by value (UNet: the whole flat buffer; WaNet: the grid head's range)
        for tag in ("alternated", "wanet"):
            _assert_reduced_generator_gradient(res, tag)


def test_data_parallel_attack_steps_two_ranks_one_gpu(tmp_path):
    """InputAwareStep and ImperceptibleStep on two ranks (tests/dp_rehearsal_attacks.py; b = 16 per rank, own images,
    second batch, labels and draws per rank).  Per class: the reduced generator gradient against the sum of the
    single-process gradients at lr_c = 0.0 -- for the input-aware step that covers the cross half reaching the
    exchange, the `_g_cross` add ordered before the one flat all-reduce and the all-reduce ordered behind both
    backward plans and their auxiliary streams; for the imperceptible step that tv_weight / n per rank with
    grad_scale = 1 / world is the mean over the global batch --, netC's reduced gradient and update at the default
    lr_c, and a second step with one poisoned image on rank 0 and none on rank 1 after which both networks'
    parameters and momentum are the same bits on both ranks.
    Measured: netC's reduced gradient against the sum of the singles 5.9e-8 (both classes), its update against the mean
    6.3e-9 / 6.9e-9; cross loss sum 4.6, TV loss sum 3.3e3 over the two steps.  9.6 s on the MI355X (the worker of
    test_data_parallel_step_two_ranks_one_gpu: 10.7 s)."""
    for res in _two_rank_rehearsal("dp_rehearsal_attacks.py", tmp_path):
        for tag, own_sum in (("inputaware", "loss_cross_sum"), ("imperceptible", "loss_tv_sum")):
            _assert_reduced_generator_gradient(res, tag)
            assert res[tag + "_gradC_sum_vs_singles"] < 1e-5, (tag, res)
            assert res[tag + "_paramC_update_vs_mean_grad"] < 1e-6, (tag, res)
            assert res[tag + "_replicas_bit_identical_after_unequal_step"] is True, (tag, res)
            assert res[tag + "_finite"] is True and res[tag + "_samples"] == 32, (tag, res)
            assert res[tag + "_" + own_sum] > 0, (tag, res)


def test_rccl_streams_beside_the_step_on_one_gpu():
    """The `nccl` backend (= RCCL) itself, on the one GPU of the box: a fresh process creates the world-size-1 group
    before any other GPU work, then runs 20 alternated steps whose bucketed gradient all-reduces are really issued
    (COMBAT_FORCE_ALLREDUCE) -- RCCL's internal streams and events beside the step's three queues, the constellation
    DESIGN.md section 5 "Schedule" measured a launch-blocking cliff for.  A one-rank sum is the identity: after one step
    the state must equal the run without a group as closely as two such runs equal each other (fp32 atomics in a few
    weight gradients: <= 1e-5), same counters.  Timing: only the launch-blocking cliff (2.5x) is
    guarded here, as <= 1.5x -- pool boxes differ by 15 % in ms/step, so a single-run 5 % bound tests the box, not the
    code; the measured ratio is printed (1.05 in round 3) and belongs to the bench record."""
    import json
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "COMBAT_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nccl_single.py"), str(port)], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("rccl world-1:", out)
    assert out["backend"] == "nccl" and out["finite"] and out["counters_equal"], out
    assert out["one_step_delta"] <= max(3 * out["one_step_noise"], 1e-7) and out["one_step_delta"] < 1e-5, out
    assert out["ms_with_rccl"] <= 1.5 * out["ms_without"] + 0.1, out


def test_c_abi_allreduce_world1():
    """SURVEY 8(b)'s `combat_allreduce(buf, count, dtype, comm, stream)`: the RCCL wrapper a non-PyTorch host binds
    (combat_comm_unique_id / _init_rank / _destroy, RCCL resolved with dlsym / dlopen at first use), exercised on the one
    GPU of the box in a fresh process (tests/rccl_cabi.py)."""
    import json
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "COMBAT_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_cabi.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["rc"] == [0, 0, 0] and out["refused"] == -1 and out["f32_identity"] and out["bf16_identity"], out


def test_bench_spawns_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` outside torchrun starts 2 ranks itself (child torch.distributed.run, gloo
    rehearsal on this one GPU) and rank 0 prints n_gpus = 2; with --full, after the golden gate."""
    import json
    env = dict(os.environ, PYTHONPATH=ROOT, COMBAT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-torch-baseline", "--no-roofline"], env=env, capture_output=True, text=True,
                       timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 256 and out["value"] > 0
    assert out["config"]["golden_gate"]["ok"]


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A plain `bench.py` run times exactly --steps steps and leaves the --full parts out of its line; with
    --dump-outputs it writes the last step's state as float32 / float64 arrays, 64 MB at most, all finite, and a
    second run with the same arguments writes the same bits (the step runs in deterministic mode)."""
    import json
    import numpy as np
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "COMBAT_DETERMINISTIC"):
        env.pop(k, None)
    dumps = []
    for run_i in range(2):
        out_dir = tmp_path / ("out%d" % run_i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "images/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert out["roofline"] is None and out["config"]["golden_gate"] is None and out["config"]["losses_finite"]
        assert out["config"]["deterministic"] is True
        assert "cpu_baseline" not in out and "pytorch_rocm_baseline" not in out
        dumps.append({f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))})
    a, b = dumps
    assert "inputs_bd.npy" in a and "metric.loss_c_sum.npy" in a and "netC.linear.weight.npy" in a
    assert any(f.startswith("netG.") for f in a)
    for f, x in a.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), f
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["inputs_bd.npy"].shape == (128, 3, 32, 32)
    # the running sums cover every step run before the dump: 2 warm-up + 3 timed steps of 128 images
    assert float(a["metric.samples.npy"]) == 128 * 5
    # the dump is the trained state, not the initial one: bench.py's seeded initial weights have moved
    import bench
    netc0, netg0, _, _ = bench.build_nets("cpu")
    for tag, net in (("netC", netc0), ("netG", netg0)):
        for k, v in net.state_dict().items():
            if k.endswith("weight") and v.numel() <= bench.DUMP_SAMPLE:
                assert not np.array_equal(a["%s.%s.npy" % (tag, k)], v.numpy()), (tag, k)
    assert sorted(a) == sorted(b)
    differ = [f for f in a if not np.array_equal(a[f], b[f])]
    assert not differ, differ
