"""The use case behind the quaternion functions, on device tensors with no host copy in between: 5000 poses arrive as
rotation matrices formed on the device, become quaternions, are normalised, are multiplied by one shared correction
quaternion and go back to rotation matrices.  Every stage's words equal the restatement's on the stage before, bit
for bit, and the rotations take every branch of arm_rotation2quaternion_f32 (a kernel with one branch fails)."""
import numpy as np
import pytest

import quaternion_ref as qr
from f32_classes import assert_same_words

ITEMS = 5000


@pytest.mark.gpu
def test_pose_chain_on_device(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(911)
    q = rng.normal(0.0, 0.35, (ITEMS, 4))
    q[np.arange(ITEMS), rng.integers(0, 4, ITEMS)] += 1.5
    q = torch.from_numpy(q.astype(np.float32)).cuda()
    # the rotations are formed on the device (torch's own arithmetic: the host reads them back below, it does not
    # form them)
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).contiguous()
    fix = torch.tensor([0.9238795, 0.0, 0.3826834, 0.0], dtype=torch.float32, device="cuda")
    nan = float("nan")
    quat = torch.full((ITEMS, 4), nan, dtype=torch.float32, device="cuda")
    unit = torch.full((ITEMS, 4), nan, dtype=torch.float32, device="cuda")
    turned = torch.full((ITEMS, 4), nan, dtype=torch.float32, device="cuda")
    back = torch.full((ITEMS, 9), nan, dtype=torch.float32, device="cuda")
    dsp.quaternion_batch("rotation2quaternion", rot, quat)
    dsp.quaternion_batch("quaternion_normalize", quat, unit)
    dsp.quaternion_product_batch(unit, fix, turned)
    dsp.quaternion_batch("quaternion2rotation", turned, back)
    torch.cuda.synchronize()
    h = rot.cpu().numpy()
    assert qr.balanced(h), np.bincount(qr.branch(h), minlength=4)
    want_q = qr.from_rotation(h)
    want_u = qr.normalize(want_q)
    want_t = qr.product(want_u, fix.cpu().numpy())
    assert_same_words(quat.cpu().numpy(), want_q, "rotation2quaternion")
    assert_same_words(unit.cpu().numpy(), want_u, "normalize")
    assert_same_words(turned.cpu().numpy(), want_t, "product with the shared quaternion")
    assert_same_words(back.cpu().numpy(), qr.to_rotation(want_t), "quaternion2rotation")
    assert not np.isnan(back.cpu().numpy()).any()
