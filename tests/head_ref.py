"""Plain torch reference of the model head (csrc/model_head.hip) for tests/test_gpu_head_fuzz.py and its CPU twin:
everything behind GlobalSumPool of the viscosity (kind 0) and the melting-point (kind 1) model, on a list of the 10 / 12
weight tensors in the packed order of impnn_model_head (include/impnn.h), in whatever dtype the tensors have.

  fp_g  = relu(pooled_g Wfp_g + bfp_g);  mixed = relu(fp_cat Wp_cat + bp_cat) + relu(fp_an Wp_an + bp_an)
  kind 0: [A, b, c] = mixed Wv + bv;  pred = A + clip(softplus(b), 0, 20) / (T / 100 + clip(softplus(c), 0.1, 50) + 1e-6)
  kind 1: pred = relu(mixed Wh + bh) Wo + bo
  loss = mean((pred - y)^2) + sum_t l2_t sum(W_t^2)

Gradients are torch autograd's.  tests/test_head_fuzz_host.py holds ``forward`` equal in fp64 to
oracle/torch_ref.py's viscosity_forward / melting_point_forward on a model without message-passing steps."""
import torch

KINDS = {"viscosity": 0, "melting_point": 1}
B_CLIP, C_CLIP = (0.0, 20.0), (0.1, 50.0)


def tensor_shapes(kind, D, F, Mx):
    """Shapes of the 10 / 12 tensors, keras layout (kernels (in, out))."""
    base = [(D, F), (F,), (D, F), (F,), (F, Mx), (Mx,), (F, Mx), (Mx,)]
    return base + ([(Mx, 3), (3,)] if kind == 0 else [(Mx, F), (F,), (F, 1), (1,)])


def softplus(x):
    """log(1 + exp(x)) without an overflow in the value or in autograd's derivative, at any x."""
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))


def forward(kind, w, pc, pa, T=None, trace=None):
    """-> pred (B,).  trace: a dict that receives the relu layers' pre-activations ("cat_fp", "an_fp", "cat_proj",
    "an_proj", kind 1: "hidden") and, kind 0, the two softplus values ("sp_b", "sp_c") and their arguments."""
    def keep(name, z):
        if trace is not None:
            trace[name] = z.detach()
        return z
    fc = torch.relu(keep("cat_fp", pc @ w[0] + w[1]))
    fa = torch.relu(keep("an_fp", pa @ w[2] + w[3]))
    mixed = torch.relu(keep("cat_proj", fc @ w[4] + w[5])) + torch.relu(keep("an_proj", fa @ w[6] + w[7]))
    if kind == 0:
        vp = mixed @ w[8] + w[9]
        keep("vp", vp)
        sp_b, sp_c = keep("sp_b", softplus(vp[:, 1])), keep("sp_c", softplus(vp[:, 2]))
        Bc, Cc = torch.clamp(sp_b, *B_CLIP), torch.clamp(sp_c, *C_CLIP)
        return vp[:, 0] + Bc / (T.reshape(-1) / 100.0 + Cc + 1e-6)
    hid = torch.relu(keep("hidden", mixed @ w[8] + w[9]))
    return (hid @ w[10] + w[11]).reshape(-1)


def loss(kind, w, pc, pa, T, y, l2, trace=None):
    """-> (loss, pred): keras "mse" plus one l2 penalty per tensor (lambda 0: none)."""
    pred = forward(kind, w, pc, pa, T, trace)
    reg = sum(float(lam) * (t ** 2).sum() for t, lam in zip(w, l2) if lam)
    return ((pred - y.reshape(-1)) ** 2).mean() + reg, pred
