"""The use case behind the classifiers, on device pointers with no host copy in between: 5000 feature vectors of
dimension 48, formed on the device, are classified by an rbf SVM with 130 support vectors and then by a 7-class
Gaussian naive Bayes model; the classes equal the restatement's, the decision values and the classes' words bit for
bit, and neither expected result is lopsided (a kernel that returns a constant fails)."""
import numpy as np
import pytest

import ml_ref as mr
from f32_classes import assert_same_words

ITEMS, DIM, NSV, CLASSES = 5000, 48, 130, 7


@pytest.mark.gpu
def test_classify_on_device(dsp, torch_gpu):
    torch = torch_gpu
    svm, _ = mr.svm_model("rbf", NSV, DIM, 0)
    bayes, _ = mr.bayes_model(CLASSES, DIM)
    bayes["theta"] = (bayes["theta"] / np.float32(6.0)).astype(np.float32)     # means inside the SVM's cube
    rng = np.random.default_rng(307)
    centre = bayes["theta"][rng.integers(0, CLASSES, ITEMS)]
    noise = rng.normal(0.0, 0.3, (ITEMS, DIM)).astype(np.float32)
    x = (torch.from_numpy(centre).cuda() + torch.from_numpy(noise).cuda()).contiguous()      # formed on the device
    # the intercept that splits a sample of these vectors in two halves (one float32 add: the host forms the same words)
    svm["intercept"] = np.float32(0)
    svm["intercept"] = np.float32(-np.median(mr.svm_sums("rbf", svm, (centre + noise)[:400]).astype(np.float64)))
    S, keep_s = dsp.svm_instance("rbf", svm["intercept"], torch.from_numpy(svm["dual"]).cuda(),
                                 torch.from_numpy(svm["sv"]).cuda(), torch.from_numpy(svm["classes"]).cuda(),
                                 gamma=float(svm["gamma"]))
    B, keep_b = dsp.bayes_instance(torch.from_numpy(bayes["theta"]).cuda(), torch.from_numpy(bayes["sigma"]).cuda(),
                                   torch.from_numpy(bayes["priors"]).cuda(), bayes["eps"])
    label = torch.full((ITEMS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    decision = torch.full((ITEMS,), float("nan"), dtype=torch.float32, device="cuda")
    prob = torch.full((ITEMS, CLASSES), float("nan"), dtype=torch.float32, device="cuda")
    cls = torch.full((ITEMS,), -1, dtype=torch.int32, device="cuda")
    dsp.svm_predict_batch("rbf", S, x, label, decision)
    dsp.bayes_predict_batch(B, x, prob, cls)
    torch.cuda.synchronize()
    hx = x.cpu().numpy()
    sums = mr.svm_sums("rbf", svm, hx)
    want = mr.svm_classes(svm, sums)
    share = [(want == c).sum() for c in svm["classes"]]
    assert min(share) * 4 >= ITEMS, share                   # each SVM class holds at least a quarter of the items
    assert np.array_equal(label.cpu().numpy(), want)
    assert_same_words(decision.cpu().numpy(), sums, "decision values")
    wprob, widx = mr.bayes_predict(bayes, hx)
    assert np.bincount(widx, minlength=CLASSES).max() * 2 <= ITEMS      # no Bayes class holds more than half
    assert_same_words(prob.cpu().numpy(), wprob, "the classes' words")
    assert np.array_equal(cls.cpu().numpy(), widx.astype(np.int32))
