"""The step list a Model runs (host only; reference: none -- there every layer is its own pass, on every call).

`compile_steps` decides ONCE which layers run together and returns one `Step` per node of the model's topological
order; Model.forward walks the list, Model._backward_pass walks it in reverse (every node of that order is reached
from an output, so every step has a consumer).  Each fusion kind is recognised here and nowhere else:

  PLAIN     the layer's own forward / backward
  FUSED     Convolutional2D / FullyConnected with the activation behind it in the epilogue, and / or with the derivative
            of the fused activation in front of it in its dx epilogue (forward_fused / backward_fused)
  ALIAS     a fused activation: its output IS its producer's (`alias_of`), its backward hands the gradient on
  PAIR      conv3x3(1->16) + LeakyReLU + conv3x3(16->1) [+ Sigmoid], one kernel each way (forward_pair / backward_pair)
  UP        Upsample2D(2) + conv on the low-res tensor (forward_up / backward_up)
  WINDOWS   windows + flatten + dense as one implicit GEMM on the conv feature map (forward_windows / backward_windows)
  ABSORBED  computed inside the PAIR / UP / WINDOWS step that names it in `inside`: no output (None), no launch
"""
import numpy as np

from .layers import (Conv2DToBatchedFixedWidthed, Convolutional2D, Flatten, FullyConnected, LeakyRelu, Sigmoid,
                     Upsample2D)

PLAIN, FUSED, ALIAS, PAIR, UP, WINDOWS, ABSORBED = 'plain', 'fused', 'alias', 'pair', 'up', 'windows', 'absorbed'


class Step:
    """kind; node: whose output it defines; layer: the conv / dense layer (PLAIN: any layer); sources: where its input
    comes from (model input numbers and node names); inside: the nodes computed within it; grad_node: the node whose
    input gradient its backward returns (`node` itself, or the first of `inside`); act / act_node: the activation in
    its epilogue; act_folded: a consumer applies that activation's derivative; in_act: the activation folded into its
    dx epilogue; first / first_act: the pair's first conv and LeakyReLU; width: of the windows; alias_of: see ALIAS."""
    __slots__ = ('kind', 'node', 'layer', 'sources', 'inside', 'grad_node', 'act', 'act_node', 'act_folded', 'in_act',
                 'first', 'first_act', 'width', 'alias_of')

    def __init__(self, kind, node, layer, sources=(), inside=(), **more):
        self.kind, self.node, self.layer, self.sources, self.inside = kind, node, layer, list(sources), tuple(inside)
        self.grad_node = inside[0] if inside else node
        self.act = self.act_node = self.in_act = self.first = self.first_act = self.width = self.alias_of = None
        self.act_folded = False
        for key, value in more.items():
            setattr(self, key, value)


class StepList:
    """steps, the maps they were made from (what Model._fusion_maps / _pairs_used / _ups_used / _wins_used show),
    output_sigmoid[k]: the fused Sigmoid behind model output k that a loss with `folds_sigmoid` may take over / None."""

    def __init__(self, steps, fused_conv, fused_act, pairs, ups, wins, output_sigmoid):
        self.steps, self.fused_conv, self.fused_act = steps, fused_conv, fused_act
        self.pairs, self.ups, self.wins, self.output_sigmoid = pairs, ups, wins, output_sigmoid


class _Graph:
    def __init__(self, layers, relations, consumers, order):
        self.layers, self.relations, self.consumers, self.order = layers, relations, consumers, order

    def only_consumer(self, node, kind):
        """The layer of type `kind` that alone consumes `node` and consumes nothing else, or None."""
        consumers = self.consumers.get(node, {})
        if len(consumers) != 1:
            return None
        (dst, _), = consumers.items()
        if isinstance(dst, int) or self.relations[dst] != [node] or not isinstance(self.layers[dst], kind):
            return None
        return dst

    def fused_input(self, node, fused_act):
        """The fused activation that feeds only `node`, or None: its backward goes into the dx epilogue of `node`'s op."""
        src = self.relations[node]
        if len(src) == 1 and src[0] in fused_act and len(self.consumers.get(src[0], {})) == 1:
            return src[0]
        return None

    def find_activations(self):
        """Every Convolutional2D / FullyConnected whose ONLY consumer is a LeakyRelu(alpha > 0) / Sigmoid runs with it
        in the epilogue.  A fused activation whose ONLY consumer is again such a layer: that layer's dx kernel
        multiplies by the activation's derivative (input_of[layer] = act), and the producer skips its own
        activation-gradient pass (the activation is folded: compile_steps)."""
        fused_conv, fused_act, input_of = {}, {}, {}
        for node in self.order:
            if not isinstance(self.layers[node], (Convolutional2D, FullyConnected)):
                continue
            dst = self.only_consumer(node, (Sigmoid, LeakyRelu))
            act = self.layers.get(dst)
            if dst is not None and type(act) in (Sigmoid, LeakyRelu) and (isinstance(act, Sigmoid) or act.alpha > 0):
                fused_conv[node] = dst
                fused_act[dst] = node
        for act_node in fused_act:
            dst = self.only_consumer(act_node, (Convolutional2D, FullyConnected))
            if dst is not None:
                input_of[dst] = act_node
        return fused_conv, fused_act, input_of

    def find_pairs(self, fused_conv, fused_act, input_of):
        """conv3x3(1->16, pad 1) + LeakyReLU feeding only conv3x3(16->1, pad 1) [+ Sigmoid] -- the Monochrome block
        (my_model/model.py:108-135) -- runs as ONE forward and ONE backward kernel (csrc/conv_pair.hip) that never
        writes the 16-channel activation or its gradient to HBM.  The kernels exist in float32 only.
        Returns {second conv: (first conv, its LeakyReLU, the second conv's fused activation or None)}."""
        pairs = {}
        for conv_b, act_a in input_of.items():
            conv_a = fused_act[act_a]
            a, b, act = self.layers[conv_a], self.layers[conv_b], self.layers[act_a]
            if not isinstance(act, LeakyRelu) or not (isinstance(a, Convolutional2D) and isinstance(b, Convolutional2D)):
                continue
            if not 0.0 <= act.alpha <= 1.0:               # the fused kernels take LeakyReLU as max(z, alpha z)
                continue
            same = all(l.kernel_size == (3, 3) and l.stride == (1, 1) and l.padding == (1, 1) for l in (a, b))
            if not (same and (a.in_channels, a.out_channels, b.in_channels, b.out_channels) == (1, 16, 16, 1)
                    and b.padding_value == 0):
                continue
            act_b = fused_conv.get(conv_b)
            if act_b is not None and not isinstance(self.layers[act_b], Sigmoid):
                continue
            pairs[conv_b] = (conv_a, act_a, act_b)
        return pairs if all(self.layers[n].w.value.dtype == np.float32 for n in pairs) else {}

    def find_ups(self, fused_act):
        """Upsample2D(2) feeding only a 5x5 / stride 1 / padding 2 Convolutional2D with 4->4 or 1->1 channels -- the
        decoder blocks of the Line and Paragraph nets (my_model/model.py:138-247) -- runs as one op on the low-res
        tensor (csrc/conv_up.hip); the upsampled tensor is never built.  float32 only, like the pair kernels.
        Returns {conv: (upsample node, fused activation that feeds only this upsample, or None)}."""
        ups = {}
        for node in self.order:
            layer = self.layers[node]
            if not isinstance(layer, Upsample2D) or tuple(layer.scale_factor) != (2, 2):
                continue
            dst = self.only_consumer(node, Convolutional2D)
            conv = self.layers.get(dst)
            if dst is not None and conv.kernel_size == (5, 5) and conv.stride == (1, 1) and conv.padding == (2, 2) \
                    and conv.padding_value == 0 and (conv.in_channels, conv.out_channels) in ((4, 4), (1, 1)) \
                    and conv.w.value.dtype == np.float32:
                ups[dst] = (node, self.fused_input(node, fused_act))
        return ups

    def find_windows(self, fused_act, shape_of):
        """Conv2DToBatchedFixedWidthed feeding only a Flatten feeding only a FullyConnected -- the bridge between the
        conv block and the dense block of the Char net (my_model/model.py:250-304) -- runs as one implicit GEMM on the
        conv feature map (ops.windows_dense_fwd): the 8x larger windows tensor and its gradient are never built.
        float32 with sizes and a channel count the MFMA implicit GEMM takes (the generic conv kernels would be slower
        than the three separate layers).
        Returns {dense: (windows node, flatten node, fused activation that feeds only the windows layer, or None)}."""
        wins = {}
        for node in self.order:
            if not isinstance(self.layers[node], Conv2DToBatchedFixedWidthed):
                continue
            flat = self.only_consumer(node, Flatten)
            dense = self.only_consumer(flat, FullyConnected) if flat is not None else None
            layer = self.layers.get(dense)
            if dense is not None and layer.is_initialized and layer.w.value.dtype == np.float32 \
                    and layer.n_output % 32 == 0 and layer.n_input % (32 * self.layers[node].width) == 0 \
                    and shape_of(self.relations[node][0])[3] % 32 == 0:
                wins[dense] = (node, flat, self.fused_input(node, fused_act))
        return wins


def compile_steps(layers, relations, consumers, order, shape_of, outputs_count, fuse_activations=False, fuse_pairs=True,
                  fuse_windows=True):
    """layers / relations / consumers (= relations_backward) / order (= _plan) of an initialised Model;
    shape_of(source) -> the shape `initialize` propagated to a model input or a node's output."""
    graph = _Graph(layers, relations, consumers, order)
    fused_conv, fused_act, input_of = graph.find_activations() if fuse_activations else ({}, {}, {})
    pairs = graph.find_pairs(fused_conv, fused_act, input_of) if fuse_activations and fuse_pairs else {}
    # nothing folds across the edge of a pair: its backward kernel applies the derivative of its own Sigmoid and of no
    # activation in front of its first conv, so that Sigmoid folds into no consumer and the activation in front keeps
    # its derivative with its producer
    pair_out = {act_b for _, _, act_b in pairs.values()} - {None}
    pair_first = {first for first, _, _ in pairs.values()}
    input_of = {dst: act for dst, act in input_of.items() if act not in pair_out and dst not in pair_first}
    foldable = {act: conv for act, conv in fused_act.items() if act not in pair_out}
    ups = graph.find_ups(foldable) if fuse_activations and fuse_pairs else {}
    wins = graph.find_windows(foldable, shape_of) if fuse_activations and fuse_windows else {}
    folded = set(input_of.values()) | {v[-1] for v in list(ups.values()) + list(wins.values()) if v[-1] is not None}
    absorbed = {n for first, act_a, _ in pairs.values() for n in (first, act_a)} | {up for up, _ in ups.values()} | \
        {n for fw, flat, _ in wins.values() for n in (fw, flat)}

    steps = []
    for node in order:
        layer = layers[node]
        act_node = fused_conv.get(node)
        epilogue = dict(act_node=act_node, act=layers.get(act_node), act_folded=act_node in folded)
        if node in absorbed:
            step = Step(ABSORBED, node, layer)
        elif node in pairs:                                # (its Sigmoid is never folded: see above)
            first, act_a, _ = pairs[node]
            step = Step(PAIR, node, layer, relations[first], (first, act_a), first=layers[first],
                        first_act=layers[act_a], **dict(epilogue, act_folded=False))
        elif node in ups:
            up, act_in = ups[node]
            step = Step(UP, node, layer, relations[up], (up,), in_act=layers.get(act_in), **epilogue)
        elif node in wins:
            fw, flat, act_in = wins[node]
            step = Step(WINDOWS, node, layer, relations[fw], (fw, flat), in_act=layers.get(act_in),
                        width=layers[fw].width, **epilogue)
        elif node in fused_act:
            step = Step(ALIAS, node, layer, alias_of=fused_act[node])
        elif node in fused_conv or node in input_of:
            step = Step(FUSED, node, layer, relations[node], in_act=layers.get(input_of.get(node)), **epilogue)
        else:
            step = Step(PLAIN, node, layer, relations[node])
        steps.append(step)

    output_sigmoid = []
    for key in range(outputs_count):
        node = relations[key][0]
        single = node in fused_act and isinstance(layers[node], Sigmoid) and len(consumers.get(node, {})) == 1
        output_sigmoid.append(node if single else None)
    return StepList(steps, fused_conv, fused_act, pairs, ups, wins, output_sigmoid)
