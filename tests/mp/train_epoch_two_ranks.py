"""Two-process data-parallel epoch (run by tests/test_train_epoch.py::test_train_epoch_two_ranks under
torch.distributed.run; one-GPU hook: both ranks on cuda:0, gloo).  Both ranks load the packed cache given as argv[1]
into a `replay.DeviceCache`, build the same DIMTrainer(group=WORLD) and run one `train_epoch` at batch 3 per rank
(global batches of 6 rows) with identically seeded generators.  The rows each rank's batches gathered are recorded
and gathered on rank 0, which checks that per global batch they are disjoint and cover the batch of the shared
permutation, and that both ranks return the same (row-weighted) epoch and batch losses.  Prints one JSON line from
rank 0."""
import json, os, sys
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
  rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
  dist.init_process_group(backend=os.environ.get("RIP_BENCH_BACKEND", "gloo"), rank=rank, world_size=world)
  dev = torch.device("cuda", 0 if os.environ.get("RIP_BENCH_SHARE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
  torch.cuda.set_device(dev)
  from oatomobile_amd import DIMTrainer, ImitativeModel, replay
  data = replay.DeviceCache(replay.PackedCache(sys.argv[1]), dev)
  seen = []
  gather = data.batch

  def recording_batch(rows, T, mode=False):
    seen.append(rows.cpu().tolist())
    return gather(rows, T, mode=mode)

  data.batch = recording_batch
  model = ImitativeModel.synthetic(500).to(dev)  # the same initial weights on every rank
  trainer = DIMTrainer(model, lr=1e-3, max_batch=4, device=dev, group=dist.group.WORLD)
  gen = torch.Generator(device=dev).manual_seed(77)
  loss = trainer.train_epoch(data, 3, generator=gen, clip=True)
  perm = trainer.last_permutation.cpu()
  n_global = (len(data) + 3 * world - 1) // (3 * world)
  seen += [[]] * (n_global - len(seen))  # an empty slice of the last global batch gathers nothing
  everything = [None] * world
  dist.all_gather_object(everything, dict(perm=perm.tolist(), seen=seen, loss=loss,
                                          losses=trainer.last_epoch_losses.cpu().tolist()))
  params = [torch.empty_like(trainer.params).cpu() for _ in range(world)]
  dist.all_gather(params, trainer.params.cpu())
  if rank == 0:
    tr = trainer._trainable.cpu().bool()
    same_perm = all(e["perm"] == everything[0]["perm"] for e in everything)
    ok = True
    for k in range(n_global):
      rows = sorted(r for e in everything for r in e["seen"][k])
      ok = ok and rows == sorted(perm[k * 3 * world:(k + 1) * 3 * world].tolist())
    print(json.dumps({"world": world, "loss": loss, "same_permutation": same_perm, "global_batches": n_global,
                      "rows_per_rank": [[len(s) for s in e["seen"]] for e in everything], "disjoint_and_cover": ok,
                      "losses_identical": all(e["loss"] == loss and e["losses"] == everything[0]["losses"]
                                              for e in everything),
                      "batch_losses": everything[0]["losses"],
                      "params_identical": all(bool(torch.equal(p[tr], params[0][tr])) for p in params)}))
  dist.barrier()
  dist.destroy_process_group()


if __name__ == "__main__":
  main()
