"""Every engine hook after every kind of evaluation: seeded walks of state-changing calls (forwards, objective evaluations, steps
of both optimizers, image / weight / precision / algorithm changes, a resample), each followed by get_blob and gram of every blob,
two ranged backwards and opfunc, with the CPU oracle beside every call (tests/sequence_oracle.py).  A hook either answers for the
image the activations belong to, within the bar the suite already holds that quantity to, or raises StError naming the blob or
the state; which (step, hook) pairs refuse is pinned by REFUSALS below, so that a refusal cannot quietly spread.

Per case two walks: 'single' runs every preparer once, 'pairs' a share of the ordered pairs of different preparers (all cases
together run all 182; tests/test_sequence_oracle_cpu.py)."""

import pytest

import sequence_oracle as so

pytestmark = pytest.mark.gpu

CASES = [(i, case, kind) for i, case in enumerate(so.cases()) for kind in ('single', 'pairs')]

# What refuses, as the walks show it: {case id: {step ("index:preparer" or "index:preparer>preparer"): {hook: what it refused}}}.
# A step that is not listed refuses nothing.  The reasons, by the state the last evaluation left:
#   * set_input / set_content / set_style / resample_input leave no valid activations: get_blob, gram and backward refuse everything
#     (until the opfunc hook, which runs last in every step, evaluates again); after resample_input alone the content has another
#     size than the iterate, and opfunc refuses too;
#   * forward_mid stops at conv2_2: the blobs above it and the backward from conv3_1 are refused;
#   * under the other weight table (set_weights) the deepest weighted blob is pool2: the same, from pool2 up;
#   * an fp32 step runs the lean forward: a pooled, un-weighted conv blob whose write the Winograd epilogue can skip (conv1_2
#     under conv algorithm 2 at these sizes; algorithm 1 skips none this small)
#     is not written -- get_blob and gram refuse it; the backwards answer (they read the arg-max maps);
#   * the lean bf16 flow ('bf16') writes no fp32 blob that only bf16 convs read: get_blob and gram refuse those, and a backward
#     that would read one as a ReLU mask or pool input is refused by backward_chain's guard, naming the blob.
SIGNATURES = {
    'S0': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 pool3 conv4_1', 'gram': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 pool3 conv4_1'},
    'S1': {'get_blob': 'conv3_2 pool3 conv4_1', 'gram': 'conv3_2 pool3 conv4_1'},
    'S2': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 pool3 conv4_1', 'gram': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 pool3 conv4_1', 'opfunc': 'opfunc'},
    'S3': {'backward': 'conv3_1+pool1+data', 'get_blob': 'pool2 conv3_1 conv3_2 pool3 conv4_1', 'gram': 'pool2 conv3_1 conv3_2 pool3 conv4_1'},
    'S4': {'backward': 'conv3_1+pool1+data', 'get_blob': 'conv3_1 conv3_2 pool3 conv4_1', 'gram': 'conv3_1 conv3_2 pool3 conv4_1'},
    'S5': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 conv3_3', 'gram': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 conv3_3'},
    'S6': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 conv3_3', 'gram': 'data conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 conv3_1 conv3_2 conv3_3', 'opfunc': 'opfunc'},
    'S7': {'backward': 'conv3_1+pool1+data', 'get_blob': 'pool2 conv3_1 conv3_2 conv3_3', 'gram': 'pool2 conv3_1 conv3_2 conv3_3'},
    'S8': {'get_blob': 'conv3_2 conv3_3', 'gram': 'conv3_2 conv3_3'},
    'S9': {'backward': 'conv3_1+pool1+data', 'get_blob': 'conv3_1 conv3_2 conv3_3', 'gram': 'conv3_1 conv3_2 conv3_3'},
    'S10': {'get_blob': 'conv1_2 conv3_2 pool3 conv4_1', 'gram': 'conv1_2 conv3_2 pool3 conv4_1'},
    'S11': {'get_blob': 'conv1_2 conv3_2 conv3_3', 'gram': 'conv1_2 conv3_2 conv3_3'},
    'S12': {'opfunc': 'opfunc'},
    'S13': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'conv1_1 conv3_2 pool3 conv4_1', 'gram': 'conv1_1 conv3_2 pool3 conv4_1'},
    'S14': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'conv1_1 conv3_1 conv3_2 pool3 conv4_1', 'gram': 'conv1_1 conv3_1 conv3_2 pool3 conv4_1'},
    'S15': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'conv1_1 conv2_1 conv3_2 conv3_3', 'gram': 'conv1_1 conv2_1 conv3_2 conv3_3'},
    'S16': {'backward': 'conv3_1+pool1+data conv2_1', 'get_blob': 'conv1_1 conv2_1 conv3_1 conv3_2 conv3_3', 'gram': 'conv1_1 conv2_1 conv3_1 conv3_2 conv3_3'},
    'S17': {'backward': 'conv3_1+pool1+data', 'get_blob': 'pool2 conv3_1 conv3_2 conv3_3', 'gram': 'pool2 conv3_1 conv3_2 conv3_3', 'opfunc': 'opfunc'},
}
REFUSALS = {
    'fp32-algo0-netA-20x28-single': {
        '0:set_algos': 'S0', '1:set_weights': 'S1', '2:set_content': 'S0', '3:step_lbfgs': 'S1', '4:set_style': 'S0',
        '5:resample_input': 'S2', '6:set_input': 'S0', '8:step_pipelined': 'S1', '9:opfunc_second': 'S1',
        '10:set_precision': 'S1', '11:forward_mid': 'S3', '12:step_adam': 'S1', '13:opfunc_first': 'S1',
    },
    'fp32-algo0-netA-20x28-pairs': {
        '0:set_content>forward_mid': 'S3', '1:opfunc_first>resample_input': 'S2', '2:set_precision>resample_input': 'S2',
        '3:set_content>opfunc_second': 'S1', '5:forward_all>set_content': 'S0', '6:step_lbfgs>set_algos': 'S1',
        '8:resample_input>step_adam': 'S1', '9:opfunc_first>forward_mid': 'S3', '10:set_algos>set_precision': 'S1',
        '12:set_style>forward_mid': 'S3',
    },
    'fp32-algo0-netA-33x65-single': {
        '0:step_pipelined': 'S1', '1:forward_mid': 'S3', '2:set_input': 'S0', '3:set_weights': 'S1', '4:set_algos': 'S4',
        '5:set_precision': 'S1', '7:opfunc_second': 'S1', '8:opfunc_first': 'S1', '9:resample_input': 'S2',
        '10:set_content': 'S0', '11:set_style': 'S0', '12:step_lbfgs': 'S1', '13:step_adam': 'S1',
    },
    'fp32-algo0-netA-33x65-pairs': {
        '0:forward_mid>set_precision': 'S3', '1:opfunc_first>step_lbfgs': 'S1', '2:set_style>opfunc_first': 'S1',
        '3:set_precision>opfunc_first': 'S1', '4:forward_mid>set_style': 'S0', '5:opfunc_second>forward_mid': 'S3',
        '6:step_lbfgs>set_precision': 'S1', '7:set_algos>step_lbfgs': 'S1', '9:set_algos>resample_input': 'S2',
        '10:step_adam>opfunc_second': 'S1', '11:set_algos>opfunc_first': 'S1', '12:step_pipelined>forward_mid': 'S3',
    },
    'fp32-algo0-netB-24x40-single': {
        '0:set_weights': 'S5', '2:resample_input': 'S6', '3:set_precision': 'S5', '4:set_content': 'S5', '5:set_input': 'S5',
        '6:forward_mid': 'S7', '7:set_style': 'S5', '8:opfunc_first': 'S8', '9:opfunc_second': 'S8', '10:step_lbfgs': 'S8',
        '11:set_algos': 'S8', '12:step_pipelined': 'S8', '13:step_adam': 'S8',
    },
    'fp32-algo0-netB-24x40-pairs': {
        '0:step_pipelined>set_precision': 'S8', '1:set_style>set_content': 'S5', '2:resample_input>step_lbfgs': 'S8',
        '3:set_content>resample_input': 'S6', '4:step_adam>set_input': 'S5', '5:set_weights>set_precision': 'S8',
        '6:step_lbfgs>resample_input': 'S6', '7:step_adam>set_content': 'S5', '8:forward_all>resample_input': 'S6',
        '9:set_style>opfunc_second': 'S8', '10:opfunc_first>step_adam': 'S8', '11:set_input>opfunc_first': 'S8',
        '12:step_adam>forward_mid': 'S7',
    },
    'fp32-algo1-netA-20x28-single': {
        '1:set_style': 'S0', '2:opfunc_second': 'S1', '3:set_precision': 'S1', '4:set_input': 'S0', '5:forward_mid': 'S3',
        '6:step_adam': 'S1', '7:step_pipelined': 'S1', '8:step_lbfgs': 'S1', '9:opfunc_first': 'S1', '10:set_content': 'S0',
        '11:set_weights': 'S1', '12:set_algos': 'S4', '13:resample_input': 'S2',
    },
    'fp32-algo1-netA-20x28-pairs': {
        '0:resample_input>set_content': 'S2', '1:set_content>set_algos': 'S0', '2:opfunc_first>set_algos': 'S1',
        '3:set_weights>set_style': 'S0', '4:opfunc_first>step_pipelined': 'S1', '5:set_precision>set_weights': 'S1',
        '6:set_weights>resample_input': 'S2', '7:set_precision>step_pipelined': 'S1', '8:set_algos>set_input': 'S0',
        '9:forward_mid>resample_input': 'S2', '11:set_input>set_algos': 'S0',
    },
    'fp32-algo1-netA-33x65-single': {
        '0:step_lbfgs': 'S1', '2:set_algos': 'S1', '3:resample_input': 'S2', '4:step_pipelined': 'S1', '5:opfunc_second': 'S1',
        '6:set_content': 'S0', '7:set_precision': 'S1', '8:set_style': 'S0', '9:step_adam': 'S1', '10:forward_mid': 'S3',
        '11:set_input': 'S0', '12:opfunc_first': 'S1', '13:set_weights': 'S1',
    },
    'fp32-algo1-netA-33x65-pairs': {
        '0:opfunc_second>opfunc_first': 'S1', '1:set_algos>set_weights': 'S1', '2:set_input>step_lbfgs': 'S1',
        '3:opfunc_second>set_precision': 'S1', '4:set_input>set_precision': 'S0', '5:step_lbfgs>set_input': 'S0',
        '7:set_content>set_style': 'S0', '8:resample_input>set_algos': 'S2', '9:opfunc_second>set_algos': 'S1',
        '10:set_content>set_weights': 'S0', '12:forward_all>forward_mid': 'S3',
    },
    'fp32-algo1-netB-24x40-single': {
        '1:step_pipelined': 'S8', '2:resample_input': 'S6', '3:opfunc_second': 'S8', '4:set_input': 'S5', '5:step_lbfgs': 'S8',
        '6:set_algos': 'S8', '7:opfunc_first': 'S8', '8:forward_mid': 'S7', '9:set_content': 'S5', '10:step_adam': 'S8',
        '11:set_precision': 'S8', '12:set_weights': 'S8', '13:set_style': 'S5',
    },
    'fp32-algo1-netB-24x40-pairs': {
        '0:step_pipelined>opfunc_second': 'S8', '1:set_algos>opfunc_second': 'S8', '2:forward_mid>set_content': 'S5',
        '3:step_lbfgs>set_style': 'S5', '4:resample_input>set_input': 'S5', '5:forward_mid>opfunc_first': 'S8',
        '6:set_precision>set_content': 'S5', '7:set_weights>opfunc_second': 'S9', '8:set_precision>forward_mid': 'S7',
        '9:opfunc_second>step_pipelined': 'S8', '10:forward_mid>set_weights': 'S7', '12:forward_all>set_style': 'S5',
    },
    'fp32-algo2-netA-20x28-single': {
        '0:forward_mid': 'S3', '1:set_input': 'S0', '2:set_precision': 'S1', '3:set_weights': 'S1', '4:set_content': 'S0',
        '5:set_style': 'S0', '6:step_lbfgs': 'S10', '7:set_algos': 'S1', '8:step_adam': 'S10', '9:resample_input': 'S2',
        '10:step_pipelined': 'S10', '12:opfunc_second': 'S1', '13:opfunc_first': 'S1',
    },
    'fp32-algo2-netA-20x28-pairs': {
        '0:set_input>set_weights': 'S0', '1:set_algos>step_pipelined': 'S1', '2:set_content>step_pipelined': 'S10',
        '3:resample_input>opfunc_second': 'S1', '4:set_style>resample_input': 'S2', '5:step_pipelined>step_adam': 'S10',
        '6:opfunc_second>step_adam': 'S10', '7:step_lbfgs>step_adam': 'S10', '8:step_lbfgs>opfunc_second': 'S1',
        '9:step_pipelined>set_content': 'S0', '10:forward_all>opfunc_second': 'S1', '11:set_weights>step_pipelined': 'S4',
        '12:step_adam>opfunc_first': 'S1',
    },
    'fp32-algo2-netB-24x40-single': {
        '0:forward_mid': 'S7', '1:set_input': 'S5', '2:set_precision': 'S8', '3:set_style': 'S5', '4:resample_input': 'S6',
        '5:step_pipelined': 'S11', '6:opfunc_second': 'S8', '7:set_content': 'S5', '9:step_lbfgs': 'S11',
        '10:opfunc_first': 'S8', '11:step_adam': 'S11', '12:set_weights': 'S8', '13:set_algos': 'S9',
    },
    'fp32-algo2-netB-24x40-pairs': {
        '0:resample_input>forward_all': 'S12', '1:opfunc_second>resample_input': 'S6', '2:set_style>step_lbfgs': 'S11',
        '3:forward_all>step_pipelined': 'S11', '4:set_precision>set_style': 'S5', '5:step_adam>set_algos': 'S11',
        '6:step_lbfgs>set_content': 'S5', '7:set_input>resample_input': 'S6', '8:opfunc_first>set_style': 'S5',
        '10:set_style>set_algos': 'S5', '11:step_adam>resample_input': 'S6', '12:set_weights>step_lbfgs': 'S9',
    },
    'bf16-algo1-netA-20x28-single': {
        '0:opfunc_first': 'S13', '1:resample_input': 'S2', '2:step_lbfgs': 'S13', '3:set_content': 'S0', '5:set_style': 'S0',
        '6:step_adam': 'S13', '7:set_weights': 'S13', '8:set_algos': 'S14', '9:opfunc_second': 'S13', '10:step_pipelined': 'S13',
        '11:set_precision': 'S13', '12:forward_mid': 'S3', '13:set_input': 'S0',
    },
    'bf16-algo1-netA-20x28-pairs': {
        '1:step_adam>set_style': 'S0', '2:step_lbfgs>set_weights': 'S13', '4:step_adam>set_precision': 'S13',
        '5:resample_input>set_style': 'S2', '6:opfunc_first>set_precision': 'S13', '7:set_precision>step_lbfgs': 'S13',
        '8:step_adam>step_pipelined': 'S13', '9:set_style>step_adam': 'S13', '10:opfunc_second>set_input': 'S0',
        '11:resample_input>opfunc_first': 'S13', '12:set_content>step_adam': 'S13',
    },
    'bf16-algo1-netA-33x65-single': {
        '0:opfunc_second': 'S13', '1:set_input': 'S0', '2:set_precision': 'S13', '3:forward_mid': 'S3', '4:step_lbfgs': 'S13',
        '5:set_algos': 'S13', '6:step_pipelined': 'S13', '7:step_adam': 'S13', '8:opfunc_first': 'S13', '9:resample_input': 'S2',
        '10:set_weights': 'S0', '11:set_content': 'S0', '12:set_style': 'S0',
    },
    'bf16-algo1-netA-33x65-pairs': {
        '0:set_input>step_pipelined': 'S13', '1:step_lbfgs>opfunc_first': 'S13', '2:step_adam>set_weights': 'S13',
        '3:forward_all>step_lbfgs': 'S13', '4:set_algos>set_content': 'S0', '5:forward_mid>step_adam': 'S13',
        '6:opfunc_first>opfunc_second': 'S13', '7:set_style>set_weights': 'S0', '8:step_pipelined>set_style': 'S0',
        '9:set_style>step_pipelined': 'S13', '10:opfunc_first>set_input': 'S0', '11:forward_mid>set_algos': 'S3',
        '12:set_content>opfunc_first': 'S13',
    },
    'bf16-algo1-netB-24x40-single': {
        '0:opfunc_first': 'S15', '1:step_pipelined': 'S15', '2:step_lbfgs': 'S15', '3:forward_mid': 'S7', '4:set_input': 'S5',
        '6:opfunc_second': 'S15', '7:set_weights': 'S15', '8:set_precision': 'S16', '9:step_adam': 'S15', '10:set_style': 'S5',
        '11:resample_input': 'S6', '12:set_algos': 'S5', '13:set_content': 'S5',
    },
    'bf16-algo1-netB-24x40-pairs': {
        '0:forward_mid>set_input': 'S7', '2:step_adam>step_lbfgs': 'S15', '3:step_lbfgs>step_pipelined': 'S15',
        '4:opfunc_second>set_content': 'S5', '5:set_input>opfunc_second': 'S15', '6:forward_all>step_adam': 'S15',
        '7:opfunc_first>set_weights': 'S15', '8:set_weights>set_input': 'S5', '9:opfunc_first>set_content': 'S5',
        '10:forward_all>opfunc_first': 'S15', '11:step_pipelined>set_algos': 'S15', '12:set_weights>set_content': 'S5',
    },
    'bf16-full-algo1-netA-20x28-single': {
        '0:step_pipelined': 'S1', '1:forward_mid': 'S3', '2:set_weights': 'S1', '3:set_content': 'S0', '4:set_input': 'S0',
        '5:opfunc_second': 'S1', '6:step_adam': 'S1', '7:step_lbfgs': 'S1', '8:opfunc_first': 'S1', '10:set_style': 'S0',
        '11:resample_input': 'S2', '12:set_algos': 'S0', '13:set_precision': 'S1',
    },
    'bf16-full-algo1-netA-20x28-pairs': {
        '0:set_weights>forward_mid': 'S3', '1:resample_input>step_pipelined': 'S1', '2:forward_mid>step_pipelined': 'S1',
        '3:set_algos>forward_mid': 'S3', '4:forward_mid>opfunc_second': 'S1', '5:set_precision>step_adam': 'S1',
        '6:step_pipelined>step_lbfgs': 'S1', '7:resample_input>set_precision': 'S2', '9:resample_input>set_weights': 'S2',
        '10:step_pipelined>opfunc_first': 'S1', '11:opfunc_second>step_lbfgs': 'S1', '12:set_precision>set_algos': 'S1',
    },
    'bf16-full-algo1-netA-33x65-single': {
        '0:step_adam': 'S1', '1:opfunc_second': 'S1', '2:step_pipelined': 'S1', '3:set_weights': 'S1', '4:set_precision': 'S4',
        '5:set_content': 'S0', '6:set_style': 'S0', '7:step_lbfgs': 'S1', '8:opfunc_first': 'S1', '9:set_input': 'S0',
        '11:set_algos': 'S1', '12:resample_input': 'S2', '13:forward_mid': 'S3',
    },
    'bf16-full-algo1-netA-33x65-pairs': {
        '0:set_input>step_adam': 'S1', '1:set_content>step_lbfgs': 'S1', '2:step_lbfgs>forward_mid': 'S3',
        '3:set_algos>set_style': 'S0', '4:opfunc_second>set_style': 'S0', '5:set_input>forward_mid': 'S3',
        '6:step_pipelined>resample_input': 'S2', '7:set_algos>step_adam': 'S1', '8:set_input>set_style': 'S0',
        '9:set_style>set_input': 'S0', '10:forward_mid>step_lbfgs': 'S1', '11:set_style>set_precision': 'S0',
        '12:set_weights>set_algos': 'S1',
    },
    'bf16-full-algo1-netB-24x40-single': {
        '0:set_precision': 'S5', '1:step_adam': 'S8', '3:set_weights': 'S8', '4:resample_input': 'S6', '5:opfunc_first': 'S8',
        '6:set_content': 'S5', '7:set_input': 'S5', '8:set_algos': 'S8', '9:step_pipelined': 'S8', '10:set_style': 'S5',
        '11:opfunc_second': 'S8', '12:step_lbfgs': 'S8', '13:forward_mid': 'S7',
    },
    'bf16-full-algo1-netB-24x40-pairs': {
        '0:set_precision>set_input': 'S5', '1:step_pipelined>set_input': 'S5', '3:set_input>set_content': 'S5',
        '4:set_weights>step_adam': 'S9', '5:set_precision>opfunc_second': 'S8', '6:step_pipelined>set_weights': 'S8',
        '8:set_weights>opfunc_first': 'S9', '9:set_content>set_precision': 'S5', '10:opfunc_second>set_weights': 'S8',
        '11:resample_input>forward_mid': 'S17', '12:set_content>set_input': 'S5',
    },
}

# After forward_all nothing may be refused, on any path; after an opfunc (first or second evaluation) on fp32 and bf16-full nothing
# but get_blob / gram of the blobs ABOVE the deepest weighted one (conv3_1), which an objective evaluation does not compute.
ABOVE_DEEPEST = {'A': 'conv3_2 pool3 conv4_1', 'B': 'conv3_2 conv3_3'}


@pytest.mark.parametrize('index,case,kind', CASES, ids=[so.case_id(c, k) for _, c, k in CASES])
def test_hooks_answer_or_refuse_after_every_call_sequence(index, case, kind):
    runner = so.Runner(case)
    try:
        refusals = runner.run(so.walk(kind, index))
    finally:
        runner.close()
    got = {}
    for step, hook, what in refusals:
        got.setdefault(step, {})[hook] = what
    print('refusals of %s: %r' % (so.case_id(case, kind), got))
    if kind == 'single':
        for step, hooks in got.items():
            name = step.split(':')[1]
            assert name != 'forward_all', 'after %s a hook refuses: %r' % (step, hooks)
            if name in ('opfunc_first', 'opfunc_second') and case[0] != 'bf16':
                assert hooks == {'get_blob': ABOVE_DEEPEST[case[2]], 'gram': ABOVE_DEEPEST[case[2]]}, 'after %s on %s: %r' % (step, case[0], hooks)
        if case[1] == 2:
            assert runner.split_checked, 'the split-operand kernel class was never asserted'
    want = {step: SIGNATURES[s] for step, s in REFUSALS.get(so.case_id(case, kind), {}).items()}
    assert got == want, 'the refusing (step, hook) pairs changed: %r' % sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
