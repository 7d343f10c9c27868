#!/usr/bin/env python3
"""tools/triplet_routes.py -- one call per route through the two fused (q, a+, a-) steps of csrc/triplet_steps.hip
(kernel family, every template argument the host chooses, where the loss is summed), and the listing that pins it.

Driven and listed exactly like tools/elementwise_routes.py, whose command line, run loop and listing it uses:
  run (on the GPU, by itself under the profiler, no counters and no other tracing):
      rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/triplet_routes.py --labels LABELS \
          [--lib LIBMMS_HIP.SO]
  listing:
      python3 tools/triplet_routes.py --listing OUT --labels LABELS > profiles/triplet_routes.txt

Every mode a call sets is back at its default when the call returns.  A call that must launch nothing (the Euclid
step beyond its generic kernel's LDS: MMS_ERR_UNSUPPORTED, asserted here) has no launches for the listing to pair
with its label, so its label ends in NO_LAUNCH and is listed alone."""
import contextlib
import io
import tempfile

import elementwise_routes as er          # parses the command line: the two scripts share it

NO_LAUNCH = " (no launch)"
N = 33                                   # three workgroups of the width-specialised kernels, the last one part full
N_TICKETS = 262145                       # at D = 100: ceil(N / 16) workgroups in ceil(./16) = 1025 groups > kTicketTop
GLOVE = (100, 200, 300)


def build_routes():
    import torch
    from mms_answer_selection_amd import capi
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(13)

    def rnd(n, D, off=0):
        """off: floats by which the tensor's base is moved off its (16-byte aligned) allocation"""
        return torch.randn(n * D + off, generator=g).to(dev)[off:].view(n, 1, D)

    def add(name, tag, D, n=N, bwd="fp32", finish="inlaunch", loss_sum="fast", want_loss=True, in_off=0, grad_off=0,
            unsupported=False):
        q, p, m = (rnd(n, D, in_off) for _ in range(3))
        dq, dp, dm = (rnd(n, D, grad_off) for _ in range(3))
        y, sp, sn = torch.ones(n, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
        loss = torch.empty(1, device=dev) if want_loss else None
        step = capi.triplet_euclid_step if name == "euclid" else capi.triplet_cosine_step

        def call():
            capi.set_euclid_backward_mode(bwd)
            capi.set_triplet_finish_mode(finish)
            capi.set_loss_sum_mode(loss_sum)
            try:
                step(q, p, m, y, sp, sn, loss, dq, dp, dm)
                assert not unsupported, "the call was served"
            except capi.MMSError as e:
                if not unsupported or "(code 2)" not in str(e):      # MMS_ERR_UNSUPPORTED
                    raise
            finally:
                capi.set_euclid_backward_mode("fp32")
                capi.set_triplet_finish_mode("inlaunch")
                capi.set_loss_sum_mode("fast")
        label = "triplet %s step %s %dx%d" % (name, tag, n, D)
        label += "".join(" %s=%s" % kv for kv in (("bwd", bwd), ("finish", finish), ("loss_sum", loss_sum))
                         if kv[1] not in ("fp32", "inlaunch", "fast"))
        label += "" if want_loss else " loss=None"
        label += " inputs +%dB" % (4 * in_off) if in_off else ""
        label += " gradients +%dB" % (4 * grad_off) if grad_off else ""
        er.ROUTES.append((label + (NO_LAUNCH if unsupported else ""), call))

    for D in GLOVE:
        for bwd in ("fp32", "reference"):
            for finish in ("inlaunch", "launch"):
                for want_loss in (True, False):
                    add("euclid", "pair32", D, bwd=bwd, finish=finish, want_loss=want_loss)
    add("euclid", "pair32", 300, loss_sum="reference")
    for tag, D in (("wave spec NIT 1", 64), ("wave spec NIT 1", 256), ("wave spec NIT 2", 400), ("wave walk NIT 2", 404),
                   ("wave walk NIT 3", 768), ("wave walk NIT 4", 1024)):
        add("euclid", tag, D)
    add("euclid", "generic (D % 4)", 30)
    add("euclid", "generic (width)", 1028)
    add("euclid", "generic (alignment)", 300, grad_off=2)
    add("euclid", "beyond the generic kernel's LDS", 1540, unsupported=True)

    for D in GLOVE:
        for finish in ("inlaunch", "launch"):
            for grad_off in (0, 2):
                add("cosine", "pair32", D, finish=finish, grad_off=grad_off)
        add("cosine", "pair32", D, want_loss=False)
    for D in (64, 400, 768, 1024):
        add("cosine", "wave NIT %d" % ((D // 4 + 63) // 64), D)
    add("cosine", "rows vec4 in (alignment of the gradients)", 64, grad_off=2)
    add("cosine", "rows vec4 in (width)", 1028)
    add("cosine", "rows scalar (D % 4)", 30)
    add("cosine", "rows scalar (alignment of the inputs)", 64, in_off=2)

    for name in ("euclid", "cosine"):
        add(name, "pair32 beyond the ticket slot", 100, n=N_TICKETS)
    return torch, capi


def listing():
    labels = open(er.args.labels).read().splitlines()
    out = io.StringIO()
    with tempfile.NamedTemporaryFile("w", suffix=".labels") as launched:
        launched.write("".join(l + "\n" for l in labels if not l.endswith(NO_LAUNCH)))
        launched.flush()
        er.args.labels = launched.name
        with contextlib.redirect_stdout(out):
            er.listing(er.args.listing)
    lines = out.getvalue().splitlines()
    for label in labels:
        if label.endswith(NO_LAUNCH):
            print(label)
        else:                                            # the label's own line, then its indented launches
            assert lines.pop(0) == label
            print(label)
            while lines and lines[0].startswith("    "):
                print(lines.pop(0))


if __name__ == "__main__":
    listing() if er.args.listing else er.run(build_routes)
