# Shared rules of the C-ABI libraries built beside liblsq_hip.so (in-tree; none links that library's objects).  A
# sub-Makefile sets
#   NAME   the library is liblsq_hip_$(NAME).so, its objects $(NAME)_<source>.o
#   SRCS   its .hip files
#   HDRS   what they include besides include/lsq_hip.h (a change to any of them rebuilds the objects)
#   LDLIBS (optional) what the library links besides the HIP runtime
# and includes this file:  make -C ml-quant_amd/csrc/<dir>  ->  ../../lib/liblsq_hip_$(NAME).so
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
ROOT    := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
OUTDIR  ?= $(ROOT)/ml-quant_amd/lib
CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fPIC -I$(ROOT)/include -Wall -Wno-unused-function
OBJS    := $(SRCS:%.hip=$(OUTDIR)/$(NAME)_%.o)
LIB     := $(OUTDIR)/liblsq_hip_$(NAME).so

all: $(LIB)

$(OUTDIR)/$(NAME)_%.o: %.hip $(HDRS) $(ROOT)/include/lsq_hip.h
	@mkdir -p $(OUTDIR)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) $(LDLIBS)

clean:
	rm -f $(OBJS) $(LIB)

.PHONY: all clean
