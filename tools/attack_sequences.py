"""What the attack states launch, recorded on the GPU: `_lib.call` is wrapped by a recorder that notes the launch and passes it through.
A launch is kept as a list: the entry point, then every argument in order -- integers and floats as they are, pointers as
't<n>:<shape>:<dtype>' with n counted by first appearance within the configuration (a pointer is the tensor `_lib.ptr` / `_lib.hptr` was
last asked for at that address; 'p<n>' for memory the recorder never saw as a tensor), an array of `_lib.ptr_array` element by element,
a host array of floats as a list, a launch descriptor as 'desc:' and the SHA-256 digest of the list of its fields (labelled the same way:
the fixture stays small).  Every tensor seen is kept alive while a configuration is recorded, so no address stands for two tensors.

    python tools/attack_sequences.py [--root DIR] OUT.json

writes the fixture tests/golden/attack_launch_sequences.json -- every distinct launch once under "launches", and per configuration the
list of their indices (`sequences_of` reads it back) --: two eager iterations of an attack state
(after one that is not recorded: the lazily built workspaces exist) at the geometry of the attack tests -- synthetic PCNet, projector
and camera 64 x 64, crop 60 x 60, ResNet-18 (and VGG-16 as second ensemble member) at input 64 x 64, three samples with mixed settings.
Recorded ONCE, from the commit before a change that must keep the launches; tests/test_attack_launches_gpu.py compares.  Only names of
spaa_amd.projector_based_attack of that commit are used, so the recorder runs on both sides of such a change.  --root: the checkout
whose spaa_amd runs.  tools/attack_digest.py prints digests of what the same configurations compute."""
import argparse
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from classifier_sequences import Recorder, _DTYPES  # noqa: E402

DEV = 'cuda'
SZ, CROP = (64, 64), (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
TARGETS, TARGETED, D_THR = [204, 291, 7], [True, True, False], [5.0, 5.0, 9.0]
LOSS = 'camdE_caml2'
ADV_LR, COL_LR, P_THRESH = 2, 1, 0.9

# name -> what differs from the plain attack on mixed settings: `clf` 'r18' or 'ens', `views` 2, per-sample `losses`, `uniform`: one
# targeted flag and one d_thr for the batch, and the keywords of the state
CONFIGS = {
    'plain-uniform': dict(uniform=True),
    'plain-mixed-prjl2': dict(losses=[LOSS, 'prjl2_caml2', LOSS]),
    'plain-f16': dict(storage='f16'),
    'ensemble': dict(clf='ens', focus=False),
    'ensemble-focus': dict(clf='ens', focus=True),
    'views': dict(views=2),
    'jitter': dict(jitter=2),
    'pose': dict(pose=2),
    'pose-jitter': dict(pose=2, jitter=2),
    'attention': dict(attention=0.25),
    'attention-ensemble': dict(clf='ens', attention=0.25),
    'transfer': dict(transfer=True),
    'transfer-views': dict(views=2, transfer=True),
    'transfer-jitter': dict(jitter=2, transfer=True),
}


class World:
    """The networks and scenes every configuration shares (built once per process)."""

    def __init__(self):
        from spaa_amd import synthetic as syn
        from spaa_amd.models import PCNet, WarpingNet
        from spaa_amd.classifier import Classifier

        def pcnet(sd):
            pc = PCNet(sd['mask'], WarpingNet(out_size=SZ))
            pc.load_state_dict(sd)
            return pc.to(DEV)

        self.pcnets = [pcnet(syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect')),
                       pcnet(syn.pcnet_state_dict(3, cam_sz=SZ, mask='rect', affine=(0.92, -0.04, -0.03, 0.05, 0.87, -0.04)))]
        self.scenes = [syn.scenes(1, 1, SZ), syn.scenes(2, 1, SZ)]
        self.r18 = Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(64, 64))
        self.vgg = Classifier('vgg16', DEV, state_dict=syn.vgg16_state_dict(3, logit_gain=5.0, fc_width=256), input_sz=(64, 64))

    def request(self, c):
        """(pcnet, classifier, cam_scene, stealth_loss, targeted, d_thr, keywords of spaa() / spaa_sweep()) of a configuration."""
        from spaa_amd import projector_based_attack as A
        views = c.get('views', 1)
        kw = {}
        if 'storage' in c:
            kw['storage'] = c['storage']
        if 'focus' in c:
            kw['focus'] = c['focus']
        if 'jitter' in c:
            kw['jitter'] = A.CaptureJitter(draws=c['jitter'], seed=1)
        if 'pose' in c:
            kw['pose'] = A.PoseJitter(draws=c['pose'], seed=1)
        if 'attention' in c:
            kw['attention'] = A.Attention(c['attention'])
        if 'transfer' in c:
            kw['transfer'] = A.Transfer(momentum=1.0, sigma=1.0)
        uni = c.get('uniform', False)
        return (self.pcnets[:views] if views > 1 else self.pcnets[0], [self.r18, self.vgg] if c.get('clf') == 'ens' else self.r18,
                self.scenes[:views] if views > 1 else self.scenes[0], LOSS if uni else c.get('losses', [LOSS] * 3),
                True if uni else TARGETED, 5.0 if uni else D_THR, kw)

    def state(self, c):
        """(the attack state of a configuration as spaa() builds it, targeted, d_thr)."""
        from spaa_amd import projector_based_attack as A
        pc, clf, sc, loss, targeted, d_thr, kw = self.request(c)
        st = A._attack_state(pc, clf, TARGETS, sc, loss, SETUP, DEV, kw.get('storage', 'f32'), kw.get('focus', False), kw.get('jitter'),
                             kw.get('attention'), kw.get('transfer'), kw.get('pose'))
        return st, targeted, d_thr


class LaunchRecorder(Recorder):
    """Recorder whose labels also tell memory it never saw as a tensor ('p<n>'), and which keeps what it saw alive."""

    def __init__(self):
        super().__init__()
        self.alive, self.unseen = [], {}

    def see(self, t):
        if t is not None:
            self.alive.append(t)
            super().see(t)

    def label(self, address):
        if address not in self.seen:
            return f'p{self.unseen.setdefault(address, len(self.unseen))}'
        shape, dtype = self.seen[address]
        n = self.labels.setdefault(address, len(self.labels))
        return f"t{n}:{'x'.join(map(str, shape))}:{_DTYPES.get(dtype) or str(dtype).replace('torch.', '')}"

    def value(self, v):
        if v is None or isinstance(v, (bool, int, float)):
            return v
        if isinstance(v, C.c_void_p):
            return None if v.value is None else self.label(v.value)
        if isinstance(v, C.Array):
            return [self.field(x, v._type_) for x in v]
        if isinstance(v, C.Structure):
            fields = [self.field(getattr(v, name), tp) for name, tp in v._fields_]
            return 'desc:' + hashlib.sha256(json.dumps(fields).encode()).hexdigest()[:16]
        if hasattr(v, '_obj'):                                     # byref(descriptor)
            return self.value(v._obj)
        if hasattr(v, 'contents'):                                 # pointer(descriptor)
            return self.value(v.contents)
        if isinstance(v, C._SimpleCData):
            return v.value
        raise TypeError(f'launch argument {v!r}')

    def field(self, v, tp):
        """An element of a ctypes array or structure: a c_void_p arrives as an integer or None."""
        if tp is C.c_void_p:
            return None if v is None else self.label(v)
        if isinstance(v, C.Structure):   # (nested in a descriptor: its fields as they are)
            return [self.field(getattr(v, name), t) for name, t in v._fields_]
        return self.value(v)


@contextlib.contextmanager
def recording(rec):
    from spaa_amd import _lib
    call, ptr, hptr = _lib.call, _lib.ptr, _lib.hptr

    def seeing(fn):
        def wrapped(t):
            rec.see(t)
            return fn(t)
        return wrapped

    def rec_call(name, *args):
        rec.seq.append([name] + [rec.value(a) for a in args])
        return call(name, *args)

    _lib.call, _lib.ptr, _lib.hptr = rec_call, seeing(ptr), seeing(hptr)
    try:
        yield
    finally:
        _lib.call, _lib.ptr, _lib.hptr = call, ptr, hptr


def record(world, c):
    """The launches of two eager iterations of a configuration, after one that is not recorded."""
    st, targeted, d_thr = world.state(c)
    st.iteration(targeted, d_thr, ADV_LR, COL_LR, P_THRESH)
    with recording(rec := LaunchRecorder()):
        for _ in range(2):
            st.iteration(targeted, d_thr, ADV_LR, COL_LR, P_THRESH)
    torch.cuda.synchronize()
    return json.loads(json.dumps(rec.seq))   # (as the fixture holds it: tuples are lists)


def sequences_of(fixture):
    """{configuration: [launch, ...]} of the loaded fixture."""
    return {name: [fixture['launches'][i] for i in index] for name, index in fixture['sequences'].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(HERE))
    ap.add_argument('out')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import spaa_amd
    from spaa_amd import _lib
    print(f'# spaa_amd from {os.path.dirname(os.path.abspath(spaa_amd.__file__))}, library {_lib.load().spaa_version().decode()}')
    world, launches, lines = World(), {}, []
    for name, c in CONFIGS.items():
        seq = record(world, c)
        index = [launches.setdefault(json.dumps(launch, separators=(",", ":")), len(launches)) for launch in seq]
        lines.append(f' {json.dumps(name)}: {json.dumps(index, separators=(",", ":"))}')
        print(name, len(seq), 'launches')
    with open(args.out, 'w') as fh:
        fh.write('{"launches": [\n' + ',\n'.join(launches) + '\n],\n"sequences": {\n' + ',\n'.join(lines) + '\n}}\n')


if __name__ == '__main__':
    main()
